"""ctypes binding of the C-ABI library (include/lc3.h, include/lc3plus_batch.h).

Nothing here computes anything: every call goes to liblc3plus_hip.so.  If the library has not been built the
import of a symbol fails loudly -- there is no Python or CPU fallback path."""
import contextlib
import ctypes as C
import os

import numpy as np

from . import packet
from .packet import *  # noqa: F401,F403  the packet layer (lc3_packet.c) lives there: its constants, plans and helpers are this module's names too
from .packet import _Egress, _FecEncode, _Receive, _RedPack, _RtpStamp, _SrtpProtect

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# every symbol include/lc3.h and include/lc3plus_batch.h declare
EXPORTS = [
    "lc3_version", "lc3_channels_supported", "lc3_samplerate_supported", "lc3_enc_get_size", "lc3_enc_init",
    "lc3_enc_set_frame_ms", "lc3_enc_set_hrmode", "lc3_enc_set_bitrate", "lc3_enc_set_bandwidth",
    "lc3_enc_get_input_samples", "lc3_enc_get_num_bytes", "lc3_enc_get_real_bitrate", "lc3_enc_get_delay",
    "lc3_enc_fl", "lc3_enc16", "lc3_enc24", "lc3_enc32", "lc3_enc_free_memory", "lc3_free_encoder_structs",
    "lc3plus_enc_batch_create", "lc3plus_enc_batch_destroy", "lc3plus_enc_batch_input_samples",
    "lc3plus_enc_batch_num_bytes", "lc3plus_enc_batch_stride", "lc3plus_enc_batch_set_bitrate",
    "lc3plus_enc_batch_set_bandwidth", "lc3plus_enc_batch_encode", "lc3plus_enc_batch_last_kernel_ms", "lc3plus_enc_batch_last_status", "lc3plus_enc_batch_last_records", "lc3plus_enc_batch_record_words", "lc3plus_enc_batch_work_buffer", "lc3plus_dec_batch_work_buffer", "lc3plus_enc_batch_set_input_ready", "lc3plus_enc_batch_state_size", "lc3plus_enc_batch_get_state", "lc3plus_enc_batch_set_state",
    "lc3plus_dec_batch_state_size", "lc3plus_dec_batch_get_state", "lc3plus_dec_batch_set_state",
    "lc3plus_enc_init", "lc3plus_enc_set_frame_ms", "lc3plus_enc_set_hrmode", "lc3plus_enc_set_bitrate",
    "lc3plus_enc16", "lc3plus_enc_get_size",
    "lc3_dec_get_size", "lc3_dec_init", "lc3_dec_set_frame_ms", "lc3_dec_set_hrmode", "lc3_dec_get_output_samples",
    "lc3_dec_get_delay", "lc3_dec_fl", "lc3_dec16", "lc3_dec24", "lc3_dec32", "lc3_dec_free_memory",
    "lc3_free_decoder_structs",
    "lc3plus_dec_batch_create", "lc3plus_dec_batch_destroy", "lc3plus_dec_batch_output_samples", "lc3plus_dec_batch_delay",
    "lc3plus_dec_batch_num_bytes", "lc3plus_dec_batch_set_num_bytes", "lc3plus_dec_batch_decode",
    "lc3plus_dec_batch_last_kernel_ms", "lc3plus_dec_batch_set_input_ready", "lc3plus_dec_batch_decode_sizes",
    "lc3plus_dec_batch_decode_sizes_device", "lc3plus_enc_batch_encode_bitrates",
    "lc3plus_enc_batch_stream_state_size", "lc3plus_enc_batch_reset_streams", "lc3plus_enc_batch_export_streams", "lc3plus_enc_batch_import_streams",
    "lc3plus_dec_batch_stream_state_size", "lc3plus_dec_batch_reset_streams", "lc3plus_dec_batch_export_streams", "lc3plus_dec_batch_import_streams",
    "lc3plus_enc_batch_encode_bandwidths", "lc3plus_enc_batch_bandwidth", "lc3plus_enc_plan_bandwidths",
    "lc3plus_enc_batch_encode_rates_device", "lc3plus_enc_plan_rates_lenient",
    "lc3plus_enc_batch_encode_packed", "lc3plus_plan_packed", "lc3plus_dec_batch_decode_packed", "lc3plus_dec_plan_packed_lenient",
    "lc3plus_pcm_format_check", "lc3plus_pcm_offset", "lc3plus_pcm_elem_bytes", "lc3plus_pcm_to_native", "lc3plus_pcm_from_native",
    "lc3plus_enc_batch_set_pcm_placement", "lc3plus_dec_batch_set_pcm_placement", "lc3plus_pcm_placed_offset", "lc3plus_plan_placed",
    "lc3plus_dec_batch_set_frame_counts", "lc3plus_dec_plan_counts",
    "lc3plus_enc_batch_set_frame_counts", "lc3plus_enc_plan_rates_ragged",
    "lc3plus_dec_batch_probe", "lc3plus_frame_info_side", "lc3plus_reject_name",
    "lc3plus_dec_batch_ingest", "lc3plus_plan_ingest",
    "lc3plus_enc_batch_egress", "lc3plus_dec_batch_egress", "lc3plus_plan_egress", "lc3plus_egress_work_bytes",
    "lc3plus_dec_batch_rtp_parse", "lc3plus_plan_rtp_parse", "lc3plus_rtp_sort_ssrc", "lc3plus_enc_batch_rtp_stamp", "lc3plus_dec_batch_rtp_stamp",
    "lc3plus_plan_rtp_stamp",
    "lc3plus_dec_batch_rtcp_stats", "lc3plus_plan_rtcp_stats", "lc3plus_rtcp_workspace_bytes",
    "lc3plus_srtp_make_context", "lc3plus_enc_batch_srtp_protect", "lc3plus_dec_batch_srtp_protect", "lc3plus_plan_srtp_protect",
    "lc3plus_dec_batch_srtp_unprotect", "lc3plus_plan_srtp_unprotect", "lc3plus_srtp_workspace_bytes",
    "lc3plus_srtp_gcm_make_context", "lc3plus_enc_batch_srtp_gcm_protect", "lc3plus_dec_batch_srtp_gcm_protect", "lc3plus_plan_srtp_gcm_protect",
    "lc3plus_dec_batch_srtp_gcm_unprotect", "lc3plus_plan_srtp_gcm_unprotect",
    "lc3plus_enc_batch_red_pack", "lc3plus_dec_batch_red_pack", "lc3plus_plan_red_pack", "lc3plus_red_work_bytes", "lc3plus_dec_batch_red_unpack",
    "lc3plus_plan_red_unpack",
    "lc3plus_enc_batch_fec_encode", "lc3plus_dec_batch_fec_encode", "lc3plus_plan_fec_encode", "lc3plus_fec_work_bytes", "lc3plus_fec_recover_work_bytes",
    "lc3plus_dec_batch_fec_recover", "lc3plus_plan_fec_recover",
    "lc3plus_dec_batch_fec_repair", "lc3plus_plan_fec_repair", "lc3plus_fec_repair_work_bytes",
    "lc3plus_shard_block",
    "lc3plus_enc_sharded_create", "lc3plus_enc_sharded_destroy", "lc3plus_enc_sharded_shards", "lc3plus_enc_sharded_shard", "lc3plus_enc_sharded_device",
    "lc3plus_enc_sharded_owner", "lc3plus_enc_sharded_input_samples", "lc3plus_enc_sharded_num_bytes", "lc3plus_enc_sharded_stride",
    "lc3plus_enc_sharded_set_bitrate", "lc3plus_enc_sharded_set_bandwidth", "lc3plus_enc_sharded_bandwidth", "lc3plus_enc_sharded_encode",
    "lc3plus_enc_sharded_encode_device", "lc3plus_enc_sharded_state_size", "lc3plus_enc_sharded_get_state", "lc3plus_enc_sharded_set_state",
    "lc3plus_enc_sharded_last_kernel_ms",
    "lc3plus_dec_sharded_create", "lc3plus_dec_sharded_destroy", "lc3plus_dec_sharded_shards", "lc3plus_dec_sharded_shard", "lc3plus_dec_sharded_device",
    "lc3plus_dec_sharded_owner", "lc3plus_dec_sharded_output_samples", "lc3plus_dec_sharded_delay", "lc3plus_dec_sharded_num_bytes",
    "lc3plus_dec_sharded_set_num_bytes", "lc3plus_dec_sharded_decode", "lc3plus_dec_sharded_decode_device", "lc3plus_dec_sharded_state_size",
    "lc3plus_dec_sharded_get_state", "lc3plus_dec_sharded_set_state", "lc3plus_dec_sharded_last_kernel_ms",
]
# the PCM format word of the batch calls (include/lc3plus_batch.h): a sample type - 16, 24, 32 or PCM_FLOAT32 - alone or with one layout
PCM_FLOAT32, PCM_INTERLEAVED, PCM_CHANNEL_MAJOR = 0x80, 0x100, 0x200
# the wire sample types: an element of 1, 2 or 3 bytes that stands for the 16- or the 24-bit integer format (big-endian, packed 24 bits, G.711)
PCM_S16_BE, PCM_S24_3LE, PCM_S24_3BE, PCM_ULAW, PCM_ALAW = 0x81, 0x82, 0x83, 0x84, 0x85
PCM_NAMES = {"s16be": PCM_S16_BE, "s24_3le": PCM_S24_3LE, "s24_3be": PCM_S24_3BE, "ulaw": PCM_ULAW, "alaw": PCM_ALAW}
PCM_LAYOUTS = {None: 0, "default": 0, "interleaved": PCM_INTERLEAVED, "channel_major": PCM_CHANNEL_MAJOR}
# flag bits of Batch.encode_device_rates (lc3plus_enc_batch_encode_rates_device)
ENC_FL_RATE, ENC_FL_BW_REFUSED, ENC_FL_BW_RANGE = 1, 2, 4
# ... and of Batch.encode_device_packed: the frame did not fit the output capacity (encoded, not written); the frame orders PACK_* of packed output: packet.py
ENC_FL_PACK_CAP = 8
# placed PCM (set_pcm_placement): the frame's PCM offset is invalid - the encoder took silence (device flags), the decoder wrote nothing (device status)
ENC_FL_PCM_PLACE, DEC_ST_PCM_PLACE = 16, 4
# per-stream frame counts (DecBatch.set_frame_counts): the frame is absent - behind its stream's count; status exactly this value, nothing decoded or written
DEC_ST_ABSENT = 8
# ... and Batch.set_frame_counts: the encoder's device flags of an absent frame are exactly this value; nothing read, encoded or written, num_bytes 0
ENC_FL_ABSENT = 32
# the frame probe (DecBatch.probe, frame_info_side; include/lc3plus_batch.h "Frame probe"): the record's words by name and its status bits, the reject reasons
# (PROBE_* and FRAME_INFO_WORDS: packet.py)
FI_STATUS, FI_REASON, FI_NUM_BYTES, FI_BW_IDX, FI_LASTNZ, FI_LSB_MODE, FI_GG_IDX, FI_FAC_NS, FI_NFILT = range(9)
FI_TNS_ORDER, FI_TNS_IDX, FI_SCF_IDX, FI_LTPF, FI_NRES = 9, 11, 27, 34, 37
FI_ST_CONCEALED, FI_ST_INVALID, FI_ST_LOST, FI_ST_SKIPPED = 1, 2, 4, 8
(REJ_NONE, REJ_BANDWIDTH, REJ_LASTNZ, REJ_SNS_INDEX_25, REJ_SNS_INDEX_24, REJ_TNS_ORDER, REJ_TNS_READER, REJ_TNS_SYMBOL, REJ_OVERLAP, REJ_SPEC_SYMBOL,
 REJ_ESCAPE_14, REJ_NRES) = range(12)
REJ_COUNT = 12
LC3_BW_WARNING = 18


class LC3Error(RuntimeError):
    def __init__(self, code, what=""):
        super().__init__("LC3_Error %d %s" % (code, what))
        self.code = code


def lib_path():
    # LC3PLUS_HIP_LIB selects another build of the same library (diagnostic builds: stage timing / stage counts)
    return os.environ.get("LC3PLUS_HIP_LIB") or os.path.join(HERE, "liblc3plus_hip.so")


def _declare_sharded(L):
    """argtypes of the sharded-batch section of include/lc3plus_batch.h (also for the stub build of the host code: tests/test_sharded_cpu.py)."""
    L.lc3plus_shard_block.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    for nm in ("lc3plus_enc_sharded", "lc3plus_dec_sharded"):
        f = lambda x: getattr(L, nm + x)
        f("_create").argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        f("_destroy").argtypes = [C.c_void_p]
        f("_shards").argtypes = [C.c_void_p]
        f("_shard").argtypes = [C.c_void_p, C.c_int]; f("_shard").restype = C.c_void_p
        f("_device").argtypes = [C.c_void_p, C.c_int]
        f("_owner").argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        f("_num_bytes").argtypes = [C.c_void_p, C.c_int]
        f("_state_size").argtypes = [C.c_void_p]; f("_state_size").restype = C.c_size_t
        f("_get_state").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        f("_set_state").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        f("_last_kernel_ms").argtypes = [C.c_void_p, C.c_int]; f("_last_kernel_ms").restype = C.c_float
    for f in ("lc3plus_enc_sharded_input_samples", "lc3plus_enc_sharded_stride", "lc3plus_dec_sharded_output_samples", "lc3plus_dec_sharded_delay"):
        getattr(L, f).argtypes = [C.c_void_p]
    for f in ("lc3plus_enc_sharded_set_bitrate", "lc3plus_enc_sharded_set_bandwidth", "lc3plus_dec_sharded_set_num_bytes"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lc3plus_enc_sharded_bandwidth.argtypes = [C.c_void_p, C.c_int]
    L.lc3plus_enc_sharded_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.lc3plus_enc_sharded_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.lc3plus_dec_sharded_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.lc3plus_dec_sharded_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]


def load_library():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError("liblc3plus_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                              "there is no fallback implementation")
        L = C.CDLL(p)
        _declare_sharded(L)
        L.lc3_enc_set_frame_ms.argtypes = [C.c_void_p, C.c_float]
        L.lc3plus_enc_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                               C.POINTER(C.c_int), C.c_int]
        L.lc3plus_enc_batch_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                               C.c_void_p, C.c_int]
        L.lc3plus_enc_batch_encode_traced.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.lc3plus_enc_batch_encode_bitrates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_enc_batch_encode_bitrates_traced.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.lc3plus_enc_plan_bitrates.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.lc3plus_enc_batch_encode_bandwidths.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                          C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_enc_batch_bandwidth.argtypes = [C.c_void_p, C.c_int]
        L.lc3plus_enc_plan_bandwidths.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.lc3plus_enc_batch_encode_rates_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_enc_plan_rates_lenient.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lc3plus_enc_batch_set_frame_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.lc3plus_enc_plan_rates_ragged.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lc3plus_enc_batch_last_kernel_ms.restype = C.c_float
        L.lc3plus_enc_batch_last_kernel_ms.argtypes = [C.c_void_p]
        L.lc3plus_enc_batch_last_status.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_enc_batch_last_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_enc_batch_work_buffer.argtypes = L.lc3plus_dec_batch_work_buffer.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.lc3plus_enc_batch_set_input_ready.argtypes = [C.c_void_p, C.c_int]
        for nm in ("lc3plus_enc_batch", "lc3plus_dec_batch"):
            getattr(L, nm + "_state_size").argtypes = [C.c_void_p]; getattr(L, nm + "_state_size").restype = C.c_size_t
            getattr(L, nm + "_get_state").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            getattr(L, nm + "_set_state").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        for nm in ("lc3plus_enc_batch", "lc3plus_dec_batch"):
            getattr(L, nm + "_stream_state_size").argtypes = [C.c_void_p]; getattr(L, nm + "_stream_state_size").restype = C.c_size_t
            getattr(L, nm + "_reset_streams").argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
            getattr(L, nm + "_export_streams").argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            getattr(L, nm + "_import_streams").argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_stream_list_check.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.lc3plus_stream_state_header.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
        L.lc3plus_stream_header_ok.argtypes = [C.c_void_p, C.c_void_p]
        for f in ("lc3plus_enc_batch_destroy", "lc3plus_enc_batch_input_samples", "lc3plus_enc_batch_stride"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.lc3plus_enc_batch_num_bytes.argtypes = [C.c_void_p, C.c_int]
        L.lc3plus_enc_batch_set_bitrate.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.lc3plus_enc_batch_set_bandwidth.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.lc3_enc_fl.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.lc3_dec_set_frame_ms.argtypes = [C.c_void_p, C.c_float]
        L.lc3_dec_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.lc3_dec_set_hrmode.argtypes = [C.c_void_p, C.c_int]
        L.lc3_dec_fl.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int]
        for f in ("lc3_dec_get_output_samples", "lc3_dec_get_delay", "lc3_free_decoder_structs"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.lc3plus_dec_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                               C.POINTER(C.c_int), C.c_int]
        L.lc3plus_dec_batch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_dec_batch_decode_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_dec_plan_sizes.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lc3plus_dec_batch_decode_sizes_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                            C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_dec_plan_sizes_lenient.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lc3plus_enc_batch_encode_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_plan_packed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lc3plus_dec_batch_decode_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_dec_plan_packed_lenient.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                      C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lc3plus_dec_batch_decode_traced.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_void_p]
        L.lc3plus_dec_batch_last_kernel_ms.restype = C.c_float
        L.lc3plus_dec_batch_last_kernel_ms.argtypes = [C.c_void_p]
        for f in ("lc3plus_dec_batch_destroy", "lc3plus_dec_batch_output_samples", "lc3plus_dec_batch_delay"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.lc3plus_dec_batch_num_bytes.argtypes = [C.c_void_p, C.c_int]
        L.lc3plus_dec_batch_set_input_ready.argtypes = [C.c_void_p, C.c_int]
        L.lc3plus_dec_batch_set_num_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.lc3plus_pcm_format_check.argtypes = [C.c_int]
        L.lc3plus_pcm_offset.argtypes = [C.c_int] * 8
        L.lc3plus_pcm_offset.restype = C.c_int64
        L.lc3plus_pcm_elem_bytes.argtypes = [C.c_int]
        for f in (L.lc3plus_pcm_to_native, L.lc3plus_pcm_from_native):
            f.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        for f in (L.lc3plus_enc_batch_set_pcm_placement, L.lc3plus_dec_batch_set_pcm_placement):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.lc3plus_pcm_placed_offset.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int]
        L.lc3plus_pcm_placed_offset.restype = C.c_int64
        L.lc3plus_plan_placed.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.lc3plus_dec_batch_set_frame_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.lc3plus_dec_plan_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        packet.declare(L)
        L.lc3plus_frame_info_side.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.lc3plus_reject_name.argtypes = [C.c_int]; L.lc3plus_reject_name.restype = C.c_char_p
        _LIB = L
    return _LIB


WORK_ELEM = {1: np.float32, 2: np.int32, 3: np.uint16, 4: np.uint8, 5: np.int64}        # LC3HIP_ELEM_* (lc3_shim.h)


def _work_buffers(fn, h):
    """the work buffers of a batch as the host runtime lists them: [(name, device pointer or None, bytes, numpy element type)]; waits for the batch's last call"""
    out = []
    name, ptr, nbytes, elem = C.c_char_p(), C.c_void_p(), C.c_size_t(), C.c_int()
    while fn(h, len(out), C.byref(name), C.byref(ptr), C.byref(nbytes), C.byref(elem)) == 0:
        out.append((name.value.decode(), ptr.value, int(nbytes.value), WORK_ELEM[elem.value]))
    return out


@contextlib.contextmanager
def launch_census():
    """The kernel launches made inside the block, as {kernel symbol name: count}: the dictionary the block receives is filled when the block ends.  A launch is
    counted on the host when the call that makes it is made, so the result is complete once the calls have returned, with sync=0 too.  Process-wide (every batch,
    every host thread): the result is the difference of the library's counts between the two ends of the block, so blocks may nest and a census of the whole
    process (LC3PLUS_LAUNCH_CENSUS) goes on undisturbed; without that switch the census is off again behind the block."""
    L = load_library()
    L.lc3hip_launch_census_read.restype = C.c_size_t
    L.lc3hip_launch_census_read.argtypes = [C.c_char_p, C.c_size_t]
    L.lc3hip_launch_census_enable.argtypes = [C.c_int]
    out = {}
    was_on = bool(os.environ.get("LC3PLUS_LAUNCH_CENSUS")) or getattr(launch_census, "depth", 0) > 0
    launch_census.depth = getattr(launch_census, "depth", 0) + 1
    L.lc3hip_launch_census_enable(1)
    before = _census_counts(L)
    try:
        yield out
    finally:
        launch_census.depth -= 1
        after = _census_counts(L)
        if not was_on:
            L.lc3hip_launch_census_enable(0)
        out.update({k: n - before.get(k, 0) for k, n in after.items() if n > before.get(k, 0)})


def _census_counts(L):
    return {name: int(n) for name, n in (line.split() for line in _census_text(L).splitlines())}


def _census_text(L):
    n = L.lc3hip_launch_census_read(None, 0)
    buf = C.create_string_buffer(n)
    L.lc3hip_launch_census_read(buf, n)
    return buf.value.decode()


def pcm_format(sample, layout=None):
    """The format word of a sample type (16, 24, 32, PCM_FLOAT32, a wire type or its name - "s16be", "s24_3le", "s24_3be", "ulaw", "alaw" - or a numpy dtype)
    and a layout (None / "default", "interleaved", "channel_major" or the bit)."""
    if isinstance(sample, str) and sample in PCM_NAMES:
        sample = PCM_NAMES[sample]
    if not isinstance(sample, int):
        dt = np.dtype(sample)
        sample = {np.dtype(np.int16): 16, np.dtype(np.float32): PCM_FLOAT32}.get(dt)
        if sample is None:
            raise ValueError("no PCM sample type for dtype %s (int32 is 24 or 32: say which)" % dt)
    word = sample | (layout if isinstance(layout, int) else PCM_LAYOUTS[layout])
    if load_library().lc3plus_pcm_format_check(word) != 0:
        raise LC3Error(1, "pcm format %#x" % word)
    return word


def pcm_shape(fmt, S, T, channels, N):
    """The array shape of one call's PCM in the layout of format word fmt."""
    tail = (3,) if (fmt & 0xFF) in (PCM_S24_3LE, PCM_S24_3BE) else ()       # packed 24 bits: uint8 with a trailing axis of the three bytes
    if fmt & PCM_INTERLEAVED:
        return (S, T * N, channels) + tail
    if fmt & PCM_CHANNEL_MAJOR:
        return (S, channels, T * N) + tail
    return (S, T, channels, N) + tail


def pcm_dtype(fmt):
    return {16: np.int16, PCM_FLOAT32: np.float32, PCM_S16_BE: np.dtype(">i2"), PCM_S24_3LE: np.uint8, PCM_S24_3BE: np.uint8, PCM_ULAW: np.uint8,
            PCM_ALAW: np.uint8}.get(fmt & 0xFF, np.int32)


def pcm_to_native(fmt, wire):
    """Wire elements (an array of pcm_dtype(fmt); packed 24 bits with a trailing axis of 3) -> the int16 / int32 they stand for (lc3plus_pcm_to_native)."""
    fmt = pcm_format(fmt & 0xFF, fmt & 0x300) if isinstance(fmt, int) else pcm_format(fmt)
    wire = np.ascontiguousarray(wire, dtype=pcm_dtype(fmt))
    p24 = (fmt & 0xFF) in (PCM_S24_3LE, PCM_S24_3BE)
    if p24 and wire.shape[-1:] != (3,):
        raise ValueError("packed 24-bit samples need a trailing axis of 3, not shape %s" % (wire.shape,))
    out = np.zeros(wire.shape[:-1] if p24 else wire.shape, dtype=np.int32 if p24 else np.int16)
    rc = load_library().lc3plus_pcm_to_native(fmt, wire.ctypes.data, out.size, out.ctypes.data) if out.size else 0
    if rc:
        raise LC3Error(rc, "lc3plus_pcm_to_native")
    return out


def pcm_from_native(fmt, native):
    """int16 (int32 for packed 24 bits) -> the wire elements the decoder would write for them, saturation included (lc3plus_pcm_from_native)."""
    fmt = pcm_format(fmt & 0xFF, fmt & 0x300) if isinstance(fmt, int) else pcm_format(fmt)
    p24 = (fmt & 0xFF) in (PCM_S24_3LE, PCM_S24_3BE)
    native = np.ascontiguousarray(native, dtype=np.int32 if p24 else np.int16)
    out = np.zeros(native.shape + ((3,) if p24 else ()), dtype=pcm_dtype(fmt))
    rc = load_library().lc3plus_pcm_from_native(fmt, native.ctypes.data, native.size, out.ctypes.data) if native.size else 0
    if rc:
        raise LC3Error(rc, "lc3plus_pcm_from_native")
    return out


def pcm_offset(fmt, channels, n_frames, samples, stream, frame, channel, sample):
    return int(load_library().lc3plus_pcm_offset(fmt, channels, n_frames, samples, stream, frame, channel, sample))


def pcm_placed_offset(fmt, channels, samples, frame_offset, channel, sample):
    """lc3plus_pcm_placed_offset: the element index of one sample of a frame placed at frame_offset, -1 for what the rule refuses."""
    return int(load_library().lc3plus_pcm_placed_offset(fmt, channels, samples, int(frame_offset), channel, sample))


def plan_placed(fmt, channels, samples, offsets, capacity):
    """lc3plus_plan_placed: uint8 array of the shape of offsets, 1 where a frame of channels * samples elements at that offset does not lie inside
    [0, capacity) - the rule the placed kernels apply to every frame."""
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    inv = np.zeros(off.shape, dtype=np.uint8)
    rc = load_library().lc3plus_plan_placed(fmt, channels, samples, off.ctypes.data if off.size else None, off.size, int(capacity),
                                            inv.ctypes.data if off.size else None)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_placed")
    return inv


def ring_offsets(starts, n_frames, ring_frames, frame_elems, ring_stride):
    """Offsets for set_pcm_placement of per-stream rings in one arena: stream s owns ring_frames slots of frame_elems elements from element
    s * ring_stride on, and the call's frame t lies in slot (starts[s] + t) % ring_frames.  int64 [n_streams, n_frames]."""
    starts = np.asarray(starts, dtype=np.int64)
    s = np.arange(starts.size, dtype=np.int64)[:, None]
    t = np.arange(n_frames, dtype=np.int64)[None, :]
    return starts[:, None] * 0 + s * int(ring_stride) + ((starts[:, None] + t) % int(ring_frames)) * int(frame_elems)


def _set_pcm_placement(obj, name, d_offsets_ptr, capacity):
    rc = getattr(obj.lib, name)(obj.h, C.c_void_p(d_offsets_ptr) if d_offsets_ptr else None, int(capacity) if d_offsets_ptr else 0)
    if rc:
        raise LC3Error(rc, name)


def _stream_list(streams):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(streams)), dtype=np.int32)


class _StreamLifecycle:
    """Reset, export and import single streams (lc3plus_{enc,dec}_batch_{reset,export,import}_streams; include/lc3plus_batch.h).  Stream lists are host
    sequences of indices; blobs are stream_state_size bytes per stream."""
    _ss = None                                                      # C prefix of the batch kind

    def _ssf(self, name):
        return getattr(self.lib, self._ss + name)

    @property
    def stream_state_size(self):
        return int(self._ssf("_stream_state_size")(self.h))

    def _reset(self, streams, config, hip_stream, sync):
        st = _stream_list(streams)
        cfg = _stream_list(config) if config is not None else None
        if cfg is not None and cfg.size != st.size:
            raise ValueError("one configuration value per listed stream")
        rc = self._ssf("_reset_streams")(self.h, st.ctypes.data, st.size, cfg.ctypes.data if cfg is not None else None,
                                          C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
        if rc:
            raise LC3Error(rc, self._ss + "_reset_streams")

    def export_streams(self, streams):
        """uint8 [n, stream_state_size]: the listed streams' blobs (returns with the data)."""
        st = _stream_list(streams)
        blob = np.zeros((st.size, self.stream_state_size), dtype=np.uint8)
        rc = self._ssf("_export_streams")(self.h, st.ctypes.data, st.size, blob.ctypes.data, 0, None, 1)
        if rc:
            raise LC3Error(rc, self._ss + "_export_streams")
        return blob

    def import_streams(self, streams, blob):
        """blob: uint8 [n, stream_state_size] from export_streams of a batch of the same codec and geometry (LC3Error where a header differs)."""
        st = _stream_list(streams)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        if blob.size != st.size * self.stream_state_size:
            raise ValueError("blob must hold %d bytes per listed stream" % self.stream_state_size)
        rc = self._ssf("_import_streams")(self.h, st.ctypes.data, st.size, blob.ctypes.data, 0, None, None, 1)
        if rc:
            raise LC3Error(rc, self._ss + "_import_streams")

    def export_streams_device(self, streams, d_ptr, hip_stream=None, sync=False):
        """The listed streams' blobs into device memory at d_ptr (16-byte aligned, n * stream_state_size bytes), queued on hip_stream."""
        st = _stream_list(streams)
        rc = self._ssf("_export_streams")(self.h, st.ctypes.data, st.size, C.c_void_p(d_ptr), 1, C.c_void_p(hip_stream) if hip_stream else None,
                                           1 if sync else 0)
        if rc:
            raise LC3Error(rc, self._ss + "_export_streams(device)")

    def import_streams_device(self, streams, d_ptr, d_status_ptr=None, hip_stream=None, sync=False):
        """Blobs from device memory at d_ptr; d_status_ptr: device uint8 [n] or None, 1 where a blob's header does not match (that stream is left as it was)."""
        st = _stream_list(streams)
        rc = self._ssf("_import_streams")(self.h, st.ctypes.data, st.size, C.c_void_p(d_ptr), 1, C.c_void_p(d_status_ptr) if d_status_ptr else None,
                                           C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
        if rc:
            raise LC3Error(rc, self._ss + "_import_streams(device)")


def stream_list_check(n_streams, streams):
    """The index-list rule of the lifecycle calls (test hook lc3plus_stream_list_check, no device needed) -> LC3_Error code."""
    st = _stream_list(streams) if streams is not None else None
    return load_library().lc3plus_stream_list_check(n_streams, st.ctypes.data if st is not None else None, st.size if st is not None else 0)


def stream_state_header(decoder, samplerate, channels, frame_ms, hrmode):
    """The blob header of a geometry (test hook lc3plus_stream_state_header) -> uint32 [4], or LC3Error where a batch would refuse the geometry."""
    h = np.zeros(4, np.uint32)
    rc = load_library().lc3plus_stream_state_header(1 if decoder else 0, samplerate, channels, frame_ms, hrmode, h.ctypes.data)
    if rc:
        raise LC3Error(rc, "lc3plus_stream_state_header")
    return h


def stream_header_ok(header, blob):
    """The header check of an import (test hook lc3plus_stream_header_ok): True where the blob starts with header."""
    h = np.ascontiguousarray(header, dtype=np.uint32)
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    assert h.size == 4 and b.size >= 16
    return bool(load_library().lc3plus_stream_header_ok(h.ctypes.data, b.ctypes.data))


class Batch(_StreamLifecycle, _Egress, _RtpStamp, _SrtpProtect, _RedPack, _FecEncode):
    """n_streams independent encoders (lc3plus_enc_batch_*), state resident on the GPU between encode() calls."""

    def __init__(self, n_streams, samplerate, channels, frame_ms, hrmode, bitrates, device=-1):
        self.lib = load_library()
        br = (C.c_int * n_streams)(*[int(b) for b in bitrates])
        self.h = C.c_void_p()
        rc = self.lib.lc3plus_enc_batch_create(C.byref(self.h), n_streams, samplerate, channels, frame_ms, hrmode, br, device)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_create")
        self.n_streams, self.channels = n_streams, channels
        self.samplerate, self.frame_ms, self.hrmode = samplerate, frame_ms, hrmode
        self.last_num_bytes = None
        self.last_result = 0          # LC3_Error of the last per-frame-bandwidth call: 0, or LC3_BW_WARNING where a value was refused (not raised)
        self.N = self.lib.lc3plus_enc_batch_input_samples(self.h)

    @classmethod
    def _borrowed(cls, lib, handle, n_streams, samplerate, channels, frame_ms, hrmode):
        """A Batch over a handle somebody else owns (a shard of a ShardedBatch): close() and the destructor leave the handle alone."""
        b = object.__new__(cls)
        b.lib, b.h, b.borrowed = lib, C.c_void_p(handle), True
        b.n_streams, b.channels = n_streams, channels
        b.samplerate, b.frame_ms, b.hrmode = samplerate, frame_ms, hrmode
        b.last_num_bytes, b.last_result = None, 0
        b.N = lib.lc3plus_enc_batch_input_samples(b.h)
        return b

    @property
    def stride(self):
        return self.lib.lc3plus_enc_batch_stride(self.h)

    def num_bytes(self, stream):
        return self.lib.lc3plus_enc_batch_num_bytes(self.h, stream)

    def set_bitrate(self, stream, bitrate):
        return self.lib.lc3plus_enc_batch_set_bitrate(self.h, stream, bitrate)

    def set_bandwidth(self, stream, bw):
        return self.lib.lc3plus_enc_batch_set_bandwidth(self.h, stream, bw)

    def bandwidth(self, stream):
        """The bandwidth in force for the stream, Hz (0: none)."""
        return self.lib.lc3plus_enc_batch_bandwidth(self.h, stream)

    def _encode_bandwidths(self, pcm_ptr, on_device, bitdepth, bandwidths, bitrates, T, out_ptr, out_stride, hip_stream, sync):
        """lc3plus_enc_batch_encode_bandwidths: bandwidths (and bitrates, or None) broadcast to [n_streams, T]; frame sizes in last_num_bytes,
        the result (0 or LC3_BW_WARNING) in last_result; any other code raises."""
        bw = np.ascontiguousarray(np.broadcast_to(np.asarray(bandwidths, dtype=np.int32), (self.n_streams, T)), dtype=np.int32)
        br = self._bitrates(bitrates, T) if bitrates is not None else None
        if br is None:
            self.last_num_bytes = np.zeros((self.n_streams, T), dtype=np.int32)
        rc = self.lib.lc3plus_enc_batch_encode_bandwidths(self.h, pcm_ptr, on_device, bitdepth, bw.ctypes.data, br.ctypes.data if br is not None else None,
                                                          T, out_ptr, out_stride, on_device, self.last_num_bytes.ctypes.data,
                                                          C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
        if rc not in (0, LC3_BW_WARNING):
            raise LC3Error(rc, "lc3plus_enc_batch_encode_bandwidths")
        self.last_result = rc

    def _bitrates(self, bitrates, T):
        """int32 [n_streams, T] per-frame bitrates, and the host buffer their frame sizes come back in (last_num_bytes)."""
        br = np.ascontiguousarray(np.broadcast_to(np.asarray(bitrates, dtype=np.int32), (self.n_streams, T)), dtype=np.int32)
        self.last_num_bytes = np.zeros((self.n_streams, T), dtype=np.int32)
        return br

    def _pcm_in(self, pcm, bitdepth, layout):
        """The format word and frame count of a host PCM array: float32 arrays are PCM_FLOAT32 whatever bitdepth says, the shape must be the layout's."""
        fmt = pcm_format(PCM_FLOAT32 if pcm.dtype == np.float32 else bitdepth & 0xFF, (bitdepth & 0x300) | (layout if isinstance(layout, int) else PCM_LAYOUTS[layout]))
        if pcm.dtype != pcm_dtype(fmt):
            raise ValueError("pcm dtype %s does not match format %#x" % (pcm.dtype, fmt))
        tail = (3,) if (fmt & 0xFF) in (PCM_S24_3LE, PCM_S24_3BE) else ()      # packed 24 bits: the three bytes of a sample
        if tail and pcm.shape[-1:] != tail:
            raise ValueError("packed 24-bit pcm needs a trailing axis of 3, not shape %s" % (pcm.shape,))
        if fmt & (PCM_INTERLEAVED | PCM_CHANNEL_MAJOR):
            n = pcm.shape[1] if fmt & PCM_INTERLEAVED else pcm.shape[2]
            T = n // self.N
            if pcm.ndim != 3 + len(tail) or n % self.N or pcm.shape != pcm_shape(fmt, self.n_streams, T, self.channels, self.N):
                raise ValueError("pcm shape %s is not %s" % (pcm.shape, "[n_streams, T * N, channels]" if fmt & PCM_INTERLEAVED else "[n_streams, channels, T * N]"))
            return fmt, T
        T = pcm.shape[1]
        if pcm.shape not in (pcm_shape(fmt, self.n_streams, T, self.channels, self.N), (self.n_streams, T, self.N) + tail if self.channels == 1 else None):
            raise ValueError("pcm shape %s is not [n_streams, T, channels, N]" % (pcm.shape,))
        return fmt, T

    def encode(self, pcm, bitdepth=16, bitrates=None, bandwidths=None, layout=None):
        """pcm: host array [n_streams, T, channels, N] (or [n_streams, T, N] for mono) -> uint8 [n_streams, T, stride].
        A float32 array is taken as PCM_FLOAT32 (full scale 1.0); layout: None, "interleaved" (pcm [n_streams, T * N, channels]) or "channel_major"
        (pcm [n_streams, channels, T * N]).  bitdepth may also be a whole format word.
        bitrates: None, or [n_streams, T] total bitrate per stream-frame (lc3plus_enc_batch_encode_bitrates): the output is then
        [n_streams, T, largest frame of the call] and last_num_bytes [n_streams, T] holds each frame's size.
        bandwidths: None, or [n_streams, T] bandwidth in Hz per stream-frame, anything that broadcasts to it (lc3plus_enc_batch_encode_bandwidths),
        with or without bitrates; last_result is then 0 or LC3_BW_WARNING (a refused value kept the bandwidth in force)."""
        pcm = np.ascontiguousarray(pcm)
        bitdepth, T = self._pcm_in(pcm, bitdepth, layout)
        if bandwidths is not None:
            stride = max(int(enc_plan_bitrates_for(self, self._bitrates(bitrates, T)).max()), 1) if bitrates is not None else self.stride
            out = np.zeros((self.n_streams, T, stride), dtype=np.uint8)
            self._encode_bandwidths(pcm.ctypes.data, 0, bitdepth, bandwidths, bitrates, T, out.ctypes.data, stride, None, True)
            return out
        if bitrates is not None:
            br = self._bitrates(bitrates, T)
            nb = enc_plan_bitrates_for(self, br)
            stride = max(int(nb.max()), 1)
            out = np.zeros((self.n_streams, T, stride), dtype=np.uint8)
            rc = self.lib.lc3plus_enc_batch_encode_bitrates(self.h, pcm.ctypes.data, 0, bitdepth, br.ctypes.data, T, out.ctypes.data, stride, 0,
                                                            self.last_num_bytes.ctypes.data, None, 1)
            if rc:
                raise LC3Error(rc, "lc3plus_enc_batch_encode_bitrates")
            return out
        stride = self.stride
        out = np.zeros((self.n_streams, T, stride), dtype=np.uint8)
        rc = self.lib.lc3plus_enc_batch_encode(self.h, pcm.ctypes.data, 0, bitdepth, T, out.ctypes.data, stride, 0, None, 1)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_encode")
        return out

    def encode_host(self, pcm, out, bitdepth=16):
        """Host buffers supplied by the caller (numpy views of pinned or pageable memory): pcm [n_streams, T, channels, N] ->
        out uint8 [n_streams, T, >= stride] in place; the library overlaps the copies with the kernels."""
        assert pcm.flags.c_contiguous and out.flags.c_contiguous and out.dtype == np.uint8
        T = pcm.shape[1]
        rc = self.lib.lc3plus_enc_batch_encode(self.h, pcm.ctypes.data, 0, bitdepth, T, out.ctypes.data, out.shape[2], 0, None, 1)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_encode(host)")
        return out

    def set_input_ready(self, ready=True):
        """Promise that the PCM of every following device-pointer call is complete when the call is made (include/lc3plus_batch.h):
        consecutive calls then overlap (the next call's frame-parallel kernels beside this call's sequential tail)."""
        rc = self.lib.lc3plus_enc_batch_set_input_ready(self.h, 1 if ready else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_set_input_ready")

    def set_pcm_placement(self, d_offsets_ptr, capacity=0):
        """lc3plus_enc_batch_set_pcm_placement: frame (s, t) of every following device-pointer call is read at element d_offsets[s, t] (int64
        [n_streams, T] in device memory) of the call's pcm pointer, a buffer of `capacity` elements; None switches placement off."""
        _set_pcm_placement(self, "lc3plus_enc_batch_set_pcm_placement", d_offsets_ptr, capacity)

    _ss = "lc3plus_enc_batch"

    def reset_streams(self, streams, bitrates=None, hip_stream=None, sync=True):
        """The listed streams start afresh; bitrates: None (configuration kept) or one total bitrate per listed stream."""
        self._reset(streams, bitrates, hip_stream, sync)

    def get_state(self):
        """The cross-frame state of all streams (opaque bytes): checkpoint for set_state() on a batch of the same configuration."""
        st = np.zeros(self.lib.lc3plus_enc_batch_state_size(self.h), dtype=np.uint8)
        rc = self.lib.lc3plus_enc_batch_get_state(self.h, st.ctypes.data, st.size)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_get_state")
        return st

    def set_state(self, st):
        st = np.ascontiguousarray(st, dtype=np.uint8)
        rc = self.lib.lc3plus_enc_batch_set_state(self.h, st.ctypes.data, st.size)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_set_state")

    def last_status(self, T):
        """uint8 [n_streams * channels, T]: LC3D_ENC_ST_* bits of the last call (0 = nothing the reference would assert on)."""
        st = np.zeros((self.n_streams * self.channels, T), dtype=np.uint8)
        n = self.lib.lc3plus_enc_batch_last_status(self.h, st.ctypes.data, st.size)
        if n < 0:
            raise LC3Error(1, "lc3plus_enc_batch_last_status")
        return st

    def last_records(self, T):
        """float32 [n_streams * channels, T, words]: the per-frame records of the last call of the pipelined path (integer fields: .view(np.int32))."""
        w = self.lib.lc3plus_enc_batch_record_words()
        rec = np.zeros((self.n_streams * self.channels, T, w), dtype=np.float32)
        n = self.lib.lc3plus_enc_batch_last_records(self.h, rec.ctypes.data, rec.size)
        if n == 0:
            raise LC3Error(1, "lc3plus_enc_batch_last_records: the last call did not take the pipelined path (it had at most 8 frames - 5 under the input-ready "
                              "promise - or was traced), so it left no records")
        if n != rec.size:
            raise LC3Error(1, "lc3plus_enc_batch_last_records (%d of %d words: T does not match the last call)" % (n, rec.size))
        return rec

    def work_buffers(self):
        """diagnostics (LC3PLUS_POISON_WORK): [(name, device pointer or None, bytes, numpy element type)] of the batch's work buffers"""
        return _work_buffers(self.lib.lc3plus_enc_batch_work_buffer, self.h)

    def encode_traced(self, pcm, bitdepth=16, bitrates=None):
        pcm = np.ascontiguousarray(pcm)
        T = pcm.shape[1]
        tsz = self.lib.lc3plus_trace_sizeof()
        traces = np.zeros((self.n_streams * self.channels * T, tsz), dtype=np.uint8)
        if bitrates is not None:
            br = self._bitrates(bitrates, T)
            self.last_num_bytes[:] = enc_plan_bitrates_for(self, br)
            stride = max(int(self.last_num_bytes.max()), 1)
            out = np.zeros((self.n_streams, T, stride), dtype=np.uint8)
            rc = self.lib.lc3plus_enc_batch_encode_bitrates_traced(self.h, pcm.ctypes.data, bitdepth, br.ctypes.data, T, out.ctypes.data, stride,
                                                                   traces.ctypes.data)
            if rc:
                raise LC3Error(rc, "lc3plus_enc_batch_encode_bitrates_traced")
            return out, traces
        stride = self.stride
        out = np.zeros((self.n_streams, T, stride), dtype=np.uint8)
        rc = self.lib.lc3plus_enc_batch_encode_traced(self.h, pcm.ctypes.data, bitdepth, T, out.ctypes.data, stride, traces.ctypes.data)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_encode_traced")
        return out, traces

    def encode_device(self, d_pcm_ptr, bitdepth, T, d_out_ptr, out_stride, hip_stream=None, sync=False, bitrates=None, bandwidths=None):
        """Device-resident variant: raw device pointers (e.g. torch tensors' data_ptr()).  bitrates, bandwidths: as for encode() (host arrays;
        last_num_bytes then holds the frame sizes)."""
        if bandwidths is not None:
            self._encode_bandwidths(C.c_void_p(d_pcm_ptr), 1, bitdepth, bandwidths, bitrates, T, C.c_void_p(d_out_ptr), out_stride, hip_stream, sync)
            return
        if bitrates is not None:
            br = self._bitrates(bitrates, T)
            rc = self.lib.lc3plus_enc_batch_encode_bitrates(self.h, C.c_void_p(d_pcm_ptr), 1, bitdepth, br.ctypes.data, T, C.c_void_p(d_out_ptr),
                                                            out_stride, 1, self.last_num_bytes.ctypes.data,
                                                            C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
            if rc:
                raise LC3Error(rc, "lc3plus_enc_batch_encode_bitrates(device)")
            return
        rc = self.lib.lc3plus_enc_batch_encode(self.h, C.c_void_p(d_pcm_ptr), 1, bitdepth, T, C.c_void_p(d_out_ptr), out_stride, 1,
                                               C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_encode(device)")

    def encode_device_rates(self, d_pcm_ptr, bitdepth, T, d_out_ptr, out_stride, d_bitrates_ptr=None, d_bandwidths_ptr=None, d_num_bytes_ptr=None,
                            d_flags_ptr=None, hip_stream=None, sync=False):
        """Per-frame rates and / or bandwidths in device memory (lc3plus_enc_batch_encode_rates_device): raw device pointers only - pcm
        [n_streams, T, channels, N], out [n_streams, T, out_stride] uint8, bitrates and bandwidths [n_streams, T] int32 (either may be None, not both),
        num_bytes [n_streams, T] int32 and flags [n_streams, T] uint8 (None or written).  Queued on hip_stream; returns at once unless sync.  A rate or
        bandwidth the host forms refuse does not fail the call: the frame keeps the carried value and is flagged (ENC_FL_*)."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_enc_batch_encode_rates_device(self.h, p(d_pcm_ptr), bitdepth, p(d_bitrates_ptr), p(d_bandwidths_ptr), T, p(d_out_ptr),
                                                            out_stride, p(d_num_bytes_ptr), p(d_flags_ptr), p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_encode_rates_device")

    def encode_device_packed(self, d_pcm_ptr, bitdepth, T, d_out_ptr, out_capacity, order=PACK_STREAM_MAJOR, d_bitrates_ptr=None,
                             d_bandwidths_ptr=None, d_offsets_ptr=None, d_total_ptr=None, d_num_bytes_ptr=None, d_flags_ptr=None, hip_stream=None,
                             sync=False):
        """Packed output in device memory (lc3plus_enc_batch_encode_packed): raw device pointers only - pcm [n_streams, T, channels, N], out
        out_capacity bytes, bitrates and bandwidths [n_streams, T] int32 (either or both may be None), offsets [n_streams, T] int64, total one int64,
        num_bytes [n_streams, T] int32 and flags [n_streams, T] uint8 (None or written).  Frame (s, t) lies at out + offsets[s, t]; order
        (PACK_STREAM_MAJOR / PACK_FRAME_MAJOR) says how the frames follow each other.  A frame past out_capacity is encoded, not written, and flagged
        ENC_FL_PACK_CAP.  Queued on hip_stream; returns at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_enc_batch_encode_packed(self.h, p(d_pcm_ptr), bitdepth, p(d_bitrates_ptr), p(d_bandwidths_ptr), T, order, p(d_out_ptr),
                                                      int(out_capacity), p(d_offsets_ptr), p(d_total_ptr), p(d_num_bytes_ptr), p(d_flags_ptr),
                                                      p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_encode_packed")

    def set_frame_counts(self, d_counts_ptr):
        """lc3plus_enc_batch_set_frame_counts: of every following encode_device_rates / encode_device_packed call stream s holds its first
        min(max(counts[s], 0), T) frames, counts an int32 [n_streams] array in device memory read when the call runs.  The frames behind them are absent -
        nothing read, encoded or written, num_bytes 0, flags ENC_FL_ABSENT - and the stream's state and configuration stop at its last present frame.  The
        other encode calls refuse while counts are set.  0 / None: off.  Only records the pointer."""
        rc = self.lib.lc3plus_enc_batch_set_frame_counts(self.h, C.c_void_p(d_counts_ptr) if d_counts_ptr else None)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_batch_set_frame_counts")

    def last_kernel_ms(self):
        return float(self.lib.lc3plus_enc_batch_last_kernel_ms(self.h))

    def close(self):
        if self.h:
            if not getattr(self, "borrowed", False):
                self.lib.lc3plus_enc_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def enc_plan_bitrates(samplerate, channels, frame_ms, hrmode, bitrates):
    """The per-frame bitrate rule of Batch.encode(bitrates=...) on the host (test hook lc3plus_enc_plan_bitrates, no device needed):
    bitrates [n_streams, n_frames] -> (num_bytes int32 [n_streams, n_frames], largest frame).  Raises LC3Error with the call's code."""
    L = load_library()
    br = np.ascontiguousarray(np.atleast_2d(np.asarray(bitrates)), dtype=np.int32)
    S, T = br.shape
    nb = np.zeros((S, T), dtype=np.int32)
    mx = C.c_int(0)
    rc = L.lc3plus_enc_plan_bitrates(samplerate, channels, frame_ms, hrmode, S, br.ctypes.data, T, nb.ctypes.data, C.byref(mx))
    if rc:
        raise LC3Error(rc, "lc3plus_enc_plan_bitrates")
    return nb, mx.value


def enc_plan_bitrates_for(batch, bitrates):
    return enc_plan_bitrates(batch.samplerate, batch.channels, batch.frame_ms, batch.hrmode, bitrates)[0]


PLAN_CHAN_WORDS = ("total_bits", "target_bits_init", "lpc_weighting", "ltpf_enable", "gg_off", "attack_handling", "reg_bits",
                   "dec_lpc_weighting", "dec_gg_off", "dec_ltpf_beta_idx")


def plan_chan(samplerate, frame_ms, hrmode, nbytes):
    """What a channel of nbytes bytes is configured with (test hook lc3plus_plan_chan, no device needed): {word: value} for PLAN_CHAN_WORDS - the encoder's
    derive_chan and the decoder's derive_dchan, the rules behind every size threshold.  Raises LC3Error (LC3_NUMBYTES_ERROR) for a size outside the range."""
    L = load_library()
    L.lc3plus_plan_chan.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]
    out = np.zeros(len(PLAN_CHAN_WORDS), dtype=np.int32)
    rc = L.lc3plus_plan_chan(samplerate, frame_ms, hrmode, int(nbytes), out.ctypes.data)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_chan")
    return dict(zip(PLAN_CHAN_WORDS, (int(x) for x in out)))


def enc_plan_bandwidths(samplerate, frame_ms, hrmode, start, bandwidths):
    """The per-frame bandwidth rule of Batch.encode(bandwidths=...) on the host (lc3plus_enc_plan_bandwidths, no device needed): start [n_streams]
    the bandwidth in force before the call, bandwidths [n_streams, n_frames] (or [n_frames] for one stream) -> (in_force int32 [n_streams, n_frames],
    0 or LC3_BW_WARNING).  Raises LC3Error with any other code."""
    L = load_library()
    bw = np.ascontiguousarray(np.atleast_2d(np.asarray(bandwidths)), dtype=np.int32)
    S, T = bw.shape
    st = np.ascontiguousarray(np.broadcast_to(np.asarray(start, dtype=np.int32), (S,)), dtype=np.int32)
    f = np.zeros((S, T), dtype=np.int32)
    rc = L.lc3plus_enc_plan_bandwidths(samplerate, frame_ms, hrmode, S, st.ctypes.data, bw.ctypes.data, T, f.ctypes.data)
    if rc not in (0, LC3_BW_WARNING):
        raise LC3Error(rc, "lc3plus_enc_plan_bandwidths")
    return f, rc


def plan_packed(sizes, order=PACK_STREAM_MAJOR, capacity=1 << 62):
    """The offsets of Batch.encode_device_packed on the host (lc3plus_plan_packed, no device needed): sizes [n_streams, n_frames] -> (LC3_Error code,
    offsets int64 [n_streams, n_frames], total, overflow uint8 [n_streams, n_frames]: ENC_FL_PACK_CAP where the frame does not fit capacity)."""
    L = load_library()
    sizes = np.ascontiguousarray(np.atleast_2d(np.asarray(sizes)), dtype=np.int32)
    S, T = sizes.shape
    offs = np.zeros((S, T), np.int64); ovf = np.zeros((S, T), np.uint8); tot = C.c_int64(0)
    rc = L.lc3plus_plan_packed(sizes.ctypes.data, S, T, int(order), int(capacity), offs.ctypes.data, C.byref(tot), ovf.ctypes.data)
    return rc, offs, tot.value, ovf


def enc_plan_rates_lenient(samplerate, channels, frame_ms, hrmode, start_rates, start_bw, bitrates=None, bandwidths=None, out_stride=1 << 20):
    """The per-frame rule of Batch.encode_device_rates on the host (test hook lc3plus_enc_plan_rates_lenient, no device needed): start_rates,
    start_bw [n_streams] the configuration before the call, bitrates / bandwidths None or [n_streams, n_frames] -> (LC3_Error code, num_bytes int32,
    bandwidth in force int32, flags uint8 [n_streams, n_frames], last rates int32 [n_streams])."""
    L = load_library()
    br = np.ascontiguousarray(np.atleast_2d(np.asarray(bitrates)), dtype=np.int32) if bitrates is not None else None
    bw = np.ascontiguousarray(np.atleast_2d(np.asarray(bandwidths)), dtype=np.int32) if bandwidths is not None else None
    S, T = (br if br is not None else bw).shape
    sr = np.ascontiguousarray(np.broadcast_to(np.asarray(start_rates, dtype=np.int32), (S,)), dtype=np.int32)
    sb = np.ascontiguousarray(np.broadcast_to(np.asarray(start_bw, dtype=np.int32), (S,)), dtype=np.int32)
    nb = np.zeros((S, T), np.int32); inf = np.zeros((S, T), np.int32); fl = np.zeros((S, T), np.uint8); end = np.zeros(S, np.int32)
    rc = L.lc3plus_enc_plan_rates_lenient(samplerate, channels, frame_ms, hrmode, S, sr.ctypes.data, sb.ctypes.data,
                                          br.ctypes.data if br is not None else None, bw.ctypes.data if bw is not None else None, T, int(out_stride),
                                          nb.ctypes.data, inf.ctypes.data, fl.ctypes.data, end.ctypes.data)
    return rc, nb, inf, fl, end


def enc_plan_rates_ragged(samplerate, channels, frame_ms, hrmode, start_rates, start_bw, bitrates=None, bandwidths=None, out_stride=1 << 20, counts=None,
                          n_frames=None):
    """enc_plan_rates_lenient with per-stream frame counts (lc3plus_enc_plan_rates_ragged, no device needed): counts None (dense) or [n_streams]; bitrates
    and bandwidths may both be None, n_frames then says how long the call is.  Absent entries: num_bytes 0, bandwidth in force 0, flags ENC_FL_ABSENT; the
    last rates are those after each stream's last present frame.  Same return as enc_plan_rates_lenient."""
    L = load_library()
    br = np.ascontiguousarray(np.atleast_2d(np.asarray(bitrates)), dtype=np.int32) if bitrates is not None else None
    bw = np.ascontiguousarray(np.atleast_2d(np.asarray(bandwidths)), dtype=np.int32) if bandwidths is not None else None
    words = br if br is not None else bw
    S, T = words.shape if words is not None else (np.asarray(start_rates).size, int(n_frames))
    sr = np.ascontiguousarray(np.broadcast_to(np.asarray(start_rates, dtype=np.int32), (S,)), dtype=np.int32)
    sb = np.ascontiguousarray(np.broadcast_to(np.asarray(start_bw, dtype=np.int32), (S,)), dtype=np.int32)
    cn = np.ascontiguousarray(np.broadcast_to(np.asarray(counts, dtype=np.int32), (S,)), dtype=np.int32) if counts is not None else None
    nb = np.zeros((S, T), np.int32); inf = np.zeros((S, T), np.int32); fl = np.zeros((S, T), np.uint8); end = np.zeros(S, np.int32)
    rc = L.lc3plus_enc_plan_rates_ragged(samplerate, channels, frame_ms, hrmode, S, sr.ctypes.data, sb.ctypes.data,
                                         br.ctypes.data if br is not None else None, bw.ctypes.data if bw is not None else None, T, int(out_stride),
                                         nb.ctypes.data, inf.ctypes.data, fl.ctypes.data, end.ctypes.data, cn.ctypes.data if cn is not None else None)
    return rc, nb, inf, fl, end


class Encoder:
    """Single-stream drop-in API (lc3_enc_*), mirrors how R/codec_exe.c:171-199,369-381 drives the reference."""

    def __init__(self, samplerate, channels=1, frame_ms=10.0, hrmode=0, bitrate=64000):
        L = self.lib = load_library()
        size = L.lc3_enc_get_size(samplerate, channels)
        if size <= 0:
            raise LC3Error(4, "lc3_enc_get_size")
        self.buf = C.create_string_buffer(size)
        self.p = C.cast(self.buf, C.c_void_p)
        self.channels = channels
        for rc, what in ((L.lc3_enc_init(self.p, samplerate, channels), "init"), (L.lc3_enc_set_frame_ms(self.p, frame_ms), "frame_ms"),
                         (L.lc3_enc_set_hrmode(self.p, hrmode), "hrmode"), (L.lc3_enc_set_bitrate(self.p, bitrate), "bitrate")):
            if rc:
                raise LC3Error(rc, what)
        self.N = L.lc3_enc_get_input_samples(self.p)
        self.nbytes = L.lc3_enc_get_num_bytes(self.p)

    def encode(self, planar, bitdepth=16):
        planar = np.ascontiguousarray(planar)
        ptrs = (C.c_void_p * self.channels)(*[planar[c].ctypes.data for c in range(self.channels)])
        out = np.zeros(self.nbytes, dtype=np.uint8)
        nb = C.c_int(0)
        rc = self.lib.lc3_enc_fl(self.p, ptrs, bitdepth, out.ctypes.data, C.byref(nb))
        if rc:
            raise LC3Error(rc, "lc3_enc_fl")
        return out[:nb.value]

    def close(self):
        if self.p:
            self.lib.lc3_free_encoder_structs(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dec_plan_sizes(samplerate, channels, frame_ms, hrmode, start, num_bytes, bfi=None, in_stride=None):
    """The per-frame size rule of DecBatch.decode(num_bytes=...) on the host (test hook lc3plus_dec_plan_sizes, no device needed):
    -> (LC3_Error code, effective sizes [S, T] uint16, lost [S, T] uint8, sizes after the call [S], largest channel frame not lost)."""
    L = load_library()
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32)
    S, T = num_bytes.shape
    start = np.ascontiguousarray(start, dtype=np.int32)
    bfi = np.ascontiguousarray(bfi, dtype=np.uint8) if bfi is not None else None
    eff = np.zeros((S, T), np.uint16); lost = np.zeros((S, T), np.uint8); end = np.zeros(S, np.int32); mx = C.c_int(0)
    rc = L.lc3plus_dec_plan_sizes(samplerate, channels, frame_ms, hrmode, S, start.ctypes.data, num_bytes.ctypes.data,
                                  bfi.ctypes.data if bfi is not None else None, T, int(in_stride if in_stride is not None else 1 << 20),
                                  eff.ctypes.data, lost.ctypes.data, end.ctypes.data, C.byref(mx))
    return rc, eff, lost, end, mx.value


def dec_plan_sizes_lenient(samplerate, channels, frame_ms, hrmode, start, num_bytes, bfi=None, in_stride=None):
    """The per-frame size rule of DecBatch.decode_device_sizes on the host (test hook lc3plus_dec_plan_sizes_lenient, no device needed): as
    dec_plan_sizes, but an invalid size or flag makes its frame lost instead of failing the call -> (LC3_Error code, effective sizes [S, T] uint16,
    lost [S, T] uint8, invalid [S, T] uint8, sizes after the call [S], largest channel frame not lost)."""
    L = load_library()
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32)
    S, T = num_bytes.shape
    start = np.ascontiguousarray(start, dtype=np.int32)
    bfi = np.ascontiguousarray(bfi, dtype=np.uint8) if bfi is not None else None
    eff = np.zeros((S, T), np.uint16); lost = np.zeros((S, T), np.uint8); inv = np.zeros((S, T), np.uint8); end = np.zeros(S, np.int32)
    mx = C.c_int(0)
    rc = L.lc3plus_dec_plan_sizes_lenient(samplerate, channels, frame_ms, hrmode, S, start.ctypes.data, num_bytes.ctypes.data,
                                          bfi.ctypes.data if bfi is not None else None, T, int(in_stride if in_stride is not None else 1 << 20),
                                          eff.ctypes.data, lost.ctypes.data, inv.ctypes.data, end.ctypes.data, C.byref(mx))
    return rc, eff, lost, inv, end, mx.value


def dec_plan_packed_lenient(samplerate, channels, frame_ms, hrmode, start, num_bytes, offsets, frames_capacity, max_frame_bytes, bfi=None):
    """The frame rule of DecBatch.decode_device_packed on the host (test hook lc3plus_dec_plan_packed_lenient, no device needed): as
    dec_plan_sizes_lenient, with each frame's offset, the buffer's capacity and the largest frame in place of in_stride -> (LC3_Error code, effective
    sizes [S, T] uint16, lost [S, T] uint8, invalid [S, T] uint8, sizes after the call [S], largest channel frame not lost)."""
    L = load_library()
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32)
    S, T = num_bytes.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    start = np.ascontiguousarray(start, dtype=np.int32)
    bfi = np.ascontiguousarray(bfi, dtype=np.uint8) if bfi is not None else None
    eff = np.zeros((S, T), np.uint16); lost = np.zeros((S, T), np.uint8); inv = np.zeros((S, T), np.uint8); end = np.zeros(S, np.int32)
    mx = C.c_int(0)
    rc = L.lc3plus_dec_plan_packed_lenient(samplerate, channels, frame_ms, hrmode, S, start.ctypes.data, num_bytes.ctypes.data, offsets.ctypes.data,
                                           int(frames_capacity), int(max_frame_bytes), bfi.ctypes.data if bfi is not None else None, T,
                                           eff.ctypes.data, lost.ctypes.data, inv.ctypes.data, end.ctypes.data, C.byref(mx))
    return rc, eff, lost, inv, end, mx.value


def dec_plan_counts(counts, n_frames):
    """The clamp of DecBatch.set_frame_counts on the host (lc3plus_dec_plan_counts, no device needed): counts [S] -> the frames of each stream present in a
    call of n_frames, int32 [S]; LC3Error for arguments the C call refuses."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    eff = np.zeros(counts.shape, np.int32)
    rc = load_library().lc3plus_dec_plan_counts(counts.ctypes.data, counts.size, int(n_frames), eff.ctypes.data)
    if rc:
        raise LC3Error(rc, "lc3plus_dec_plan_counts")
    return eff


def reject_names():
    """the names of REJ_* by code, as the library gives them (lc3plus_reject_name): ("none", "bandwidth", ...)"""
    L = load_library()
    return tuple(L.lc3plus_reject_name(i).decode() for i in range(REJ_COUNT))


def frame_info_side(samplerate, channels, frame_ms, hrmode, frame):
    """The SIDE depth of DecBatch.probe on the host (lc3plus_frame_info_side, no device needed): one stream-frame (bytes, all channels; empty = lost) ->
    int32 [channels, FRAME_INFO_WORDS]; LC3Error for a geometry the C call refuses."""
    frame = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
    info = np.zeros((channels, FRAME_INFO_WORDS), np.int32)
    rc = load_library().lc3plus_frame_info_side(samplerate, channels, frame_ms, hrmode, frame.ctypes.data if frame.size else None, int(frame.size),
                                                info.ctypes.data)
    if rc:
        raise LC3Error(rc, "lc3plus_frame_info_side")
    return info


class DecBatch(_StreamLifecycle, _Receive, _Egress, _RtpStamp, _SrtpProtect, _RedPack, _FecEncode):
    """n_streams independent decoders (lc3plus_dec_batch_*), state resident on the GPU between decode() calls."""

    def __init__(self, n_streams, samplerate, channels, frame_ms, hrmode, num_bytes, device=-1):
        """num_bytes: bytes per stream-frame of every stream, or None (sizes set later or passed with the frames)."""
        self.lib = load_library()
        nb = (C.c_int * n_streams)(*[int(b) for b in num_bytes]) if num_bytes is not None else None
        self.h = C.c_void_p()
        rc = self.lib.lc3plus_dec_batch_create(C.byref(self.h), n_streams, samplerate, channels, frame_ms, hrmode, nb, device)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_create")
        self.n_streams, self.channels = n_streams, channels
        self.N = self.lib.lc3plus_dec_batch_output_samples(self.h)

    _ss = "lc3plus_dec_batch"

    @classmethod
    def _borrowed(cls, lib, handle, n_streams, channels):
        """A DecBatch over a handle somebody else owns (a shard of a ShardedDecBatch)."""
        b = object.__new__(cls)
        b.lib, b.h, b.borrowed = lib, C.c_void_p(handle), True
        b.n_streams, b.channels = n_streams, channels
        b.N = lib.lc3plus_dec_batch_output_samples(b.h)
        return b

    def num_bytes(self, stream):
        return self.lib.lc3plus_dec_batch_num_bytes(self.h, stream)

    def reset_streams(self, streams, num_bytes=None, hip_stream=None, sync=True):
        """The listed streams start afresh; num_bytes: None (sizes kept) or one stream-frame size per listed stream."""
        self._reset(streams, num_bytes, hip_stream, sync)

    def set_num_bytes(self, stream, nbytes):
        return self.lib.lc3plus_dec_batch_set_num_bytes(self.h, stream, nbytes)

    def get_state(self):
        """The decoders' cross-frame state (opaque bytes): checkpoint for set_state() on a batch of the same configuration."""
        st = np.zeros(self.lib.lc3plus_dec_batch_state_size(self.h), dtype=np.uint8)
        rc = self.lib.lc3plus_dec_batch_get_state(self.h, st.ctypes.data, st.size)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_get_state")
        return st

    def set_state(self, st):
        st = np.ascontiguousarray(st, dtype=np.uint8)
        rc = self.lib.lc3plus_dec_batch_set_state(self.h, st.ctypes.data, st.size)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_set_state")

    def _prep(self, frames, bfi, bps, layout=None):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        S, T, stride = frames.shape
        assert S == self.n_streams
        if bfi is not None:
            bfi = np.ascontiguousarray(bfi, dtype=np.uint8)
            assert bfi.shape == (S, T)
        fmt = pcm_format(bps & 0xFF, (bps & 0x300) | (layout if isinstance(layout, int) else PCM_LAYOUTS[layout]))
        pcm = np.zeros(pcm_shape(fmt, S, T, self.channels, self.N), dtype=pcm_dtype(fmt))
        status = np.zeros((S, T), dtype=np.uint8)
        return frames, T, stride, bfi, pcm, status

    def _sizes(self, num_bytes, T):
        num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32)
        if num_bytes.shape != (self.n_streams, T):                 # the C call reads n_streams * T entries
            raise ValueError("num_bytes must have shape %s, not %s" % ((self.n_streams, T), num_bytes.shape))
        return num_bytes

    def decode(self, frames, bfi=None, bps=16, num_bytes=None, layout=None):
        """frames: uint8 [n_streams, T, stride]; bfi: optional [n_streams, T] -> (pcm [n_streams, T, channels, N], status).
        num_bytes: optional [n_streams, T] bytes of every stream-frame, 0 = lost (lc3plus_dec_batch_decode_sizes).
        bps: 16, 24, 32 or PCM_FLOAT32 (float32 samples, full scale 1.0), or a whole format word; layout: None, "interleaved" (pcm [n_streams, T * N,
        channels]) or "channel_major" (pcm [n_streams, channels, T * N])."""
        bps = pcm_format(bps & 0xFF, (bps & 0x300) | (layout if isinstance(layout, int) else PCM_LAYOUTS[layout]))
        frames, T, stride, bfi, pcm, status = self._prep(frames, bfi, bps)
        if num_bytes is not None:
            nb = self._sizes(num_bytes, T)
            rc = self.lib.lc3plus_dec_batch_decode_sizes(self.h, frames.ctypes.data, 0, stride, nb.ctypes.data, bfi.ctypes.data if bfi is not None else None,
                                                         T, pcm.ctypes.data, 0, bps, status.ctypes.data, None, 1)
            if rc:
                raise LC3Error(rc, "lc3plus_dec_batch_decode_sizes")
            return pcm, status
        rc = self.lib.lc3plus_dec_batch_decode(self.h, frames.ctypes.data, 0, stride, bfi.ctypes.data if bfi is not None else None, T,
                                               pcm.ctypes.data, 0, bps, status.ctypes.data, None, 1)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_decode")
        return pcm, status

    def decode_device_sizes(self, d_frames_ptr, in_stride, T, d_pcm_ptr, d_num_bytes_ptr, d_bfi_ptr=None, d_status_ptr=None, bps=16, hip_stream=None,
                            sync=False):
        """Per-frame sizes and flags in device memory (lc3plus_dec_batch_decode_sizes_device): raw device pointers only - frames [n_streams, T, in_stride]
        uint8, num_bytes [n_streams, T] int32 (0 = lost), optional bfi [n_streams, T] uint8 and status [n_streams, T] uint8, pcm [n_streams, T, channels, N].
        Queued on hip_stream; returns at once unless sync.  An invalid size or flag conceals its frame (status bit 1) instead of failing the call."""
        rc = self.lib.lc3plus_dec_batch_decode_sizes_device(self.h, C.c_void_p(d_frames_ptr), in_stride, C.c_void_p(d_num_bytes_ptr),
                                                            C.c_void_p(d_bfi_ptr) if d_bfi_ptr else None, T, C.c_void_p(d_pcm_ptr), bps,
                                                            C.c_void_p(d_status_ptr) if d_status_ptr else None,
                                                            C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_decode_sizes_device")

    def decode_device_packed(self, d_frames_ptr, frames_capacity, d_offsets_ptr, T, d_pcm_ptr, d_num_bytes_ptr, max_frame_bytes, d_bfi_ptr=None,
                             d_status_ptr=None, bps=16, hip_stream=None, sync=False):
        """Frames packed back to back in device memory (lc3plus_dec_batch_decode_packed): raw device pointers only - frames frames_capacity bytes,
        offsets [n_streams, T] int64, num_bytes [n_streams, T] int32 (0 = lost), optional bfi and status [n_streams, T] uint8, pcm [n_streams, T,
        channels, N].  A frame outside the buffer or above max_frame_bytes is concealed (status bit 1) and never read.  Queued on hip_stream; returns
        at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_dec_batch_decode_packed(self.h, p(d_frames_ptr), int(frames_capacity), p(d_offsets_ptr), p(d_num_bytes_ptr),
                                                      int(max_frame_bytes), p(d_bfi_ptr), T, p(d_pcm_ptr), bps, p(d_status_ptr), p(hip_stream),
                                                      1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_decode_packed")

    def decode_traced(self, frames, bfi=None, bps=16):
        frames, T, stride, bfi, pcm, status = self._prep(frames, bfi, bps)
        tsz = self.lib.lc3plus_dec_trace_sizeof()
        traces = np.zeros((self.n_streams * self.channels * T, tsz), dtype=np.uint8)
        rc = self.lib.lc3plus_dec_batch_decode_traced(self.h, frames.ctypes.data, stride, bfi.ctypes.data if bfi is not None else None, T,
                                                      pcm.ctypes.data, bps, status.ctypes.data, traces.ctypes.data)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_decode_traced")
        return pcm, status, traces

    def set_input_ready(self, ready=True):
        """lc3plus_dec_batch_set_input_ready: the frames of every following device-pointer call are complete on the device when the call is made."""
        rc = self.lib.lc3plus_dec_batch_set_input_ready(self.h, 1 if ready else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_set_input_ready")

    def set_pcm_placement(self, d_offsets_ptr, capacity=0):
        """lc3plus_dec_batch_set_pcm_placement: frame (s, t) of every following device-pointer call is written at element d_offsets[s, t] (int64
        [n_streams, T] in device memory) of the call's pcm pointer, a buffer of `capacity` elements; None switches placement off."""
        _set_pcm_placement(self, "lc3plus_dec_batch_set_pcm_placement", d_offsets_ptr, capacity)

    def set_frame_counts(self, d_counts_ptr):
        """lc3plus_dec_batch_set_frame_counts: of every following decode_device_sizes / decode_device_packed call stream s holds its first
        min(max(d_counts[s], 0), T) frames (int32 [n_streams] in device memory, read when the call runs); the frames behind them are absent - nothing read,
        decoded, concealed or written, status DEC_ST_ABSENT - and the stream's state stops at its last present frame.  The other decode calls refuse while
        counts are set; None switches them off."""
        rc = self.lib.lc3plus_dec_batch_set_frame_counts(self.h, C.c_void_p(d_counts_ptr) if d_counts_ptr else None)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_set_frame_counts")

    def decode_device(self, d_frames_ptr, in_stride, T, d_pcm_ptr, bps=16, hip_stream=None, sync=False, num_bytes=None, bfi=None):
        """Device-resident variant: raw device pointers.  Without num_bytes no bad-frame flags; with num_bytes ([n_streams, T] host ints, 0 = lost)
        and optional host bfi the ordered per-frame-size call (lc3plus_dec_batch_decode_sizes), which returns when it is done."""
        if num_bytes is not None:
            nb = self._sizes(num_bytes, T)
            if bfi is not None:
                bfi = np.ascontiguousarray(bfi, dtype=np.uint8)
                if bfi.shape != (self.n_streams, T):
                    raise ValueError("bfi must have shape %s, not %s" % ((self.n_streams, T), bfi.shape))
            rc = self.lib.lc3plus_dec_batch_decode_sizes(self.h, C.c_void_p(d_frames_ptr), 1, in_stride, nb.ctypes.data,
                                                         bfi.ctypes.data if bfi is not None else None, T, C.c_void_p(d_pcm_ptr), 1, bps, None,
                                                         C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
            if rc:
                raise LC3Error(rc, "lc3plus_dec_batch_decode_sizes(device)")
            return
        rc = self.lib.lc3plus_dec_batch_decode(self.h, C.c_void_p(d_frames_ptr), 1, in_stride, None, T, C.c_void_p(d_pcm_ptr), 1, bps, None,
                                               C.c_void_p(hip_stream) if hip_stream else None, 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_decode(device)")

    def last_kernel_ms(self):
        return float(self.lib.lc3plus_dec_batch_last_kernel_ms(self.h))

    def work_buffers(self):
        """as Batch.work_buffers"""
        return _work_buffers(self.lib.lc3plus_dec_batch_work_buffer, self.h)

    def close(self):
        if self.h:
            if not getattr(self, "borrowed", False):
                self.lib.lc3plus_dec_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_block(n_streams, n_shards, shard, lib=None):
    """(first, count) of the streams shard `shard` of `n_shards` owns (lc3plus_shard_block, no device needed); LC3Error for arguments it refuses."""
    first, count = C.c_int(0), C.c_int(0)
    rc = (lib or load_library()).lc3plus_shard_block(n_streams, n_shards, shard, C.byref(first), C.byref(count))
    if rc:
        raise LC3Error(rc, "lc3plus_shard_block")
    return first.value, count.value


def _ptr_array(ptrs, n):
    """n raw pointers (ints or None) as a C array of void*; None for no list."""
    if ptrs is None:
        return None
    ptrs = list(ptrs)
    if len(ptrs) != n:
        raise ValueError("one pointer per shard (%d), not %d" % (n, len(ptrs)))
    return (C.c_void_p * n)(*[C.c_void_p(int(p)) if p else None for p in ptrs])


class _Sharded:
    """What ShardedBatch and ShardedDecBatch share: the shards, their blocks and the checkpoint calls (lc3plus_{enc,dec}_sharded_*)."""
    _sp = None                                                      # C prefix

    def _f(self, name):
        return getattr(self.lib, self._sp + name)

    def _create(self, n_streams, samplerate, channels, frame_ms, hrmode, config, devices, lib):
        self.lib = lib or load_library()
        cfg = np.ascontiguousarray(config, dtype=np.int32) if config is not None else None
        if cfg is not None and cfg.size != n_streams:
            raise ValueError("one configuration value per stream")
        dev = np.ascontiguousarray(devices, dtype=np.int32) if devices is not None else None
        self.h = C.c_void_p()
        rc = self._f("_create")(C.byref(self.h), n_streams, samplerate, channels, frame_ms, hrmode, cfg.ctypes.data if cfg is not None else None,
                                dev.ctypes.data if dev is not None else None, dev.size if dev is not None else 0)
        if rc:
            self.h = None
            raise LC3Error(rc, self._sp + "_create")
        self.n_streams, self.channels = n_streams, channels
        self.samplerate, self.frame_ms, self.hrmode = samplerate, frame_ms, hrmode
        self.n_shards = self._f("_shards")(self.h)
        self.devices = [self._f("_device")(self.h, i) for i in range(self.n_shards)]
        self.blocks = [shard_block(n_streams, self.n_shards, i, self.lib) for i in range(self.n_shards)]

    def owner(self, stream):
        """(shard, local index) of a global stream index."""
        k, l = C.c_int(0), C.c_int(0)
        rc = self._f("_owner")(self.h, stream, C.byref(k), C.byref(l))
        if rc:
            raise LC3Error(rc, self._sp + "_owner")
        return k.value, l.value

    def num_bytes(self, stream):
        return self._f("_num_bytes")(self.h, stream)

    @property
    def state_size(self):
        return int(self._f("_state_size")(self.h))

    def get_state(self):
        """The shards' states one after the other: the state of an unsharded batch of n_streams (and of a sharded one with any number of shards)."""
        st = np.zeros(self.state_size, dtype=np.uint8)
        rc = self._f("_get_state")(self.h, st.ctypes.data, st.size)
        if rc:
            raise LC3Error(rc, self._sp + "_get_state")
        return st

    def set_state(self, st):
        st = np.ascontiguousarray(st, dtype=np.uint8)
        rc = self._f("_set_state")(self.h, st.ctypes.data, st.size)
        if rc:
            raise LC3Error(rc, self._sp + "_set_state")

    def last_kernel_ms(self, shard):
        return float(self._f("_last_kernel_ms")(self.h, shard))

    def close(self):
        if getattr(self, "h", None):
            self._f("_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedBatch(_Sharded):
    """n_streams encoders in contiguous blocks over devices (lc3plus_enc_sharded_*; one shard per entry of devices, the same device may appear more than
    once).  Stream indices are global; encode() takes and returns what Batch.encode() does, byte for byte."""
    _sp = "lc3plus_enc_sharded"

    def __init__(self, n_streams, samplerate, channels, frame_ms, hrmode, bitrates, devices, lib=None):
        self._create(n_streams, samplerate, channels, frame_ms, hrmode, bitrates, devices, lib)
        self.last_num_bytes, self.last_result = None, 0
        self.N = self.lib.lc3plus_enc_sharded_input_samples(self.h)

    _pcm_in = Batch._pcm_in
    _bitrates = Batch._bitrates

    def shard(self, i):
        """The shard's Batch, borrowed: local stream indices (owner()); closing it leaves the shard alone."""
        h = self.lib.lc3plus_enc_sharded_shard(self.h, i)
        if not h:
            raise LC3Error(1, "lc3plus_enc_sharded_shard")
        return Batch._borrowed(self.lib, h, self.blocks[i][1], self.samplerate, self.channels, self.frame_ms, self.hrmode)

    @property
    def stride(self):
        return self.lib.lc3plus_enc_sharded_stride(self.h)

    def set_bitrate(self, stream, bitrate):
        return self.lib.lc3plus_enc_sharded_set_bitrate(self.h, stream, bitrate)

    def set_bandwidth(self, stream, bw):
        return self.lib.lc3plus_enc_sharded_set_bandwidth(self.h, stream, bw)

    def bandwidth(self, stream):
        return self.lib.lc3plus_enc_sharded_bandwidth(self.h, stream)

    def encode(self, pcm, bitdepth=16, bitrates=None, bandwidths=None, layout=None):
        """As Batch.encode: pcm over all n_streams -> uint8 [n_streams, T, stride]; last_num_bytes [n_streams, T]; last_result 0 or LC3_BW_WARNING."""
        pcm = np.ascontiguousarray(pcm)
        fmt, T = self._pcm_in(pcm, bitdepth, layout)
        br = self._bitrates(bitrates, T) if bitrates is not None else None
        bw = np.ascontiguousarray(np.broadcast_to(np.asarray(bandwidths, dtype=np.int32), (self.n_streams, T)), dtype=np.int32) if bandwidths is not None else None
        stride = max(int(enc_plan_bitrates_for(self, br).max()), 1) if br is not None else self.stride
        if br is None:
            self.last_num_bytes = np.zeros((self.n_streams, T), dtype=np.int32)
        out = np.zeros((self.n_streams, T, stride), dtype=np.uint8)
        rc = self.lib.lc3plus_enc_sharded_encode(self.h, pcm.ctypes.data, fmt, bw.ctypes.data if bw is not None else None,
                                                 br.ctypes.data if br is not None else None, T, out.ctypes.data, stride, self.last_num_bytes.ctypes.data)
        if rc not in (0, LC3_BW_WARNING):
            raise LC3Error(rc, "lc3plus_enc_sharded_encode")
        self.last_result = rc
        return out

    def encode_device(self, d_pcm_ptrs, bitdepth, T, d_out_ptrs, out_stride, hip_streams=None, sync=False):
        """Raw device pointers, one per shard, each on its shard's device and holding that shard's block.  Every shard's call is queued before any is
        waited for; returns after queueing unless sync."""
        rc = self.lib.lc3plus_enc_sharded_encode_device(self.h, _ptr_array(d_pcm_ptrs, self.n_shards), bitdepth, T, _ptr_array(d_out_ptrs, self.n_shards),
                                                        out_stride, _ptr_array(hip_streams, self.n_shards), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_enc_sharded_encode_device")


class ShardedDecBatch(_Sharded):
    """n_streams decoders in contiguous blocks over devices (lc3plus_dec_sharded_*); decode() takes and returns what DecBatch.decode() does."""
    _sp = "lc3plus_dec_sharded"

    def __init__(self, n_streams, samplerate, channels, frame_ms, hrmode, num_bytes, devices, lib=None):
        self._create(n_streams, samplerate, channels, frame_ms, hrmode, num_bytes, devices, lib)
        self.N = self.lib.lc3plus_dec_sharded_output_samples(self.h)

    _prep = DecBatch._prep
    _sizes = DecBatch._sizes

    def shard(self, i):
        """The shard's DecBatch, borrowed: local stream indices (owner())."""
        h = self.lib.lc3plus_dec_sharded_shard(self.h, i)
        if not h:
            raise LC3Error(1, "lc3plus_dec_sharded_shard")
        return DecBatch._borrowed(self.lib, h, self.blocks[i][1], self.channels)

    @property
    def delay(self):
        return self.lib.lc3plus_dec_sharded_delay(self.h)

    def set_num_bytes(self, stream, nbytes):
        return self.lib.lc3plus_dec_sharded_set_num_bytes(self.h, stream, nbytes)

    def decode(self, frames, bfi=None, bps=16, num_bytes=None, layout=None):
        """As DecBatch.decode: frames uint8 [n_streams, T, stride] -> (pcm, status)."""
        bps = pcm_format(bps & 0xFF, (bps & 0x300) | (layout if isinstance(layout, int) else PCM_LAYOUTS[layout]))
        frames, T, stride, bfi, pcm, status = self._prep(frames, bfi, bps)
        nb = self._sizes(num_bytes, T) if num_bytes is not None else None
        rc = self.lib.lc3plus_dec_sharded_decode(self.h, frames.ctypes.data, stride, nb.ctypes.data if nb is not None else None,
                                                 bfi.ctypes.data if bfi is not None else None, T, pcm.ctypes.data, bps, status.ctypes.data)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_sharded_decode")
        return pcm, status

    def decode_device(self, d_frames_ptrs, in_stride, T, d_pcm_ptrs, bps=16, hip_streams=None, sync=False):
        """Raw device pointers, one per shard, as ShardedBatch.encode_device."""
        rc = self.lib.lc3plus_dec_sharded_decode_device(self.h, _ptr_array(d_frames_ptrs, self.n_shards), in_stride, T, _ptr_array(d_pcm_ptrs, self.n_shards),
                                                        bps, _ptr_array(hip_streams, self.n_shards), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_sharded_decode_device")


class Decoder:
    """Single-stream drop-in API (lc3_dec_*), used exactly as R/codec_exe.c uses the reference decoder."""

    def __init__(self, samplerate, channels=1, frame_ms=10.0, hrmode=0):
        self.lib = load_library()
        size = self.lib.lc3_dec_get_size(samplerate, channels)
        if size <= 0:
            raise LC3Error(1, "lc3_dec_get_size")
        self.buf = C.create_string_buffer(size)
        self.h = C.cast(self.buf, C.c_void_p)
        self.channels = channels
        for rc, what in ((self.lib.lc3_dec_init(self.h, samplerate, channels, 0), "lc3_dec_init"),
                         (self.lib.lc3_dec_set_frame_ms(self.h, frame_ms), "lc3_dec_set_frame_ms"),
                         (self.lib.lc3_dec_set_hrmode(self.h, hrmode), "lc3_dec_set_hrmode")):
            if rc:
                raise LC3Error(rc, what)
        self.N = self.lib.lc3_dec_get_output_samples(self.h)

    def decode(self, frame, bfi_ext=0, bps=16):
        """frame: bytes of one stream-frame -> (planar samples [channels, N], LC3_Error code 0 or 2)."""
        data = np.frombuffer(bytes(frame), dtype=np.uint8).copy() if len(frame) else np.zeros(1, dtype=np.uint8)
        out = np.zeros((self.channels, self.N), dtype=np.int16 if bps == 16 else np.int32)
        ptrs = (C.c_void_p * self.channels)(*[out[c].ctypes.data for c in range(self.channels)])
        rc = self.lib.lc3_dec_fl(self.h, data.ctypes.data, len(frame), ptrs, bps, bfi_ext)
        if rc not in (0, 2):
            raise LC3Error(rc, "lc3_dec_fl")
        return out, rc

    def close(self):
        if self.h:
            self.lib.lc3_free_decoder_structs(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
