"""ctypes binding of the C-ABI library (include/lc3.h, include/lc3plus_batch.h).

Nothing here computes anything: every call goes to liblc3plus_hip.so.  If the library has not been built the
import of a symbol fails loudly -- there is no Python or CPU fallback path."""
import contextlib
import ctypes as C
import os
import types

import numpy as np

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
# ... and of Batch.encode_device_packed: the frame did not fit the output capacity (encoded, not written); the frame orders of packed output
ENC_FL_PACK_CAP = 8
# placed PCM (set_pcm_placement): the frame's PCM offset is invalid - the encoder took silence (device flags), the decoder wrote nothing (device status)
ENC_FL_PCM_PLACE, DEC_ST_PCM_PLACE = 16, 4
# per-stream frame counts (DecBatch.set_frame_counts): the frame is absent - behind its stream's count; status exactly this value, nothing decoded or written
DEC_ST_ABSENT = 8
# ... and Batch.set_frame_counts: the encoder's device flags of an absent frame are exactly this value; nothing read, encoded or written, num_bytes 0
ENC_FL_ABSENT = 32
PACK_STREAM_MAJOR, PACK_FRAME_MAJOR = 0, 1
# the frame probe (DecBatch.probe, frame_info_side; include/lc3plus_batch.h "Frame probe"): depths, the record's words and status bits, the reject reasons
PROBE_SIDE, PROBE_FULL = 0, 1
FRAME_INFO_WORDS = 48
FI_STATUS, FI_REASON, FI_NUM_BYTES, FI_BW_IDX, FI_LASTNZ, FI_LSB_MODE, FI_GG_IDX, FI_FAC_NS, FI_NFILT = range(9)
FI_TNS_ORDER, FI_TNS_IDX, FI_SCF_IDX, FI_LTPF, FI_NRES = 9, 11, 27, 34, 37
FI_ST_CONCEALED, FI_ST_INVALID, FI_ST_LOST, FI_ST_SKIPPED = 1, 2, 4, 8
(REJ_NONE, REJ_BANDWIDTH, REJ_LASTNZ, REJ_SNS_INDEX_25, REJ_SNS_INDEX_24, REJ_TNS_ORDER, REJ_TNS_READER, REJ_TNS_SYMBOL, REJ_OVERLAP, REJ_SPEC_SYMBOL,
 REJ_ESCAPE_14, REJ_NRES) = range(12)
REJ_COUNT = 12
# packet ingest (DecBatch.ingest, plan_ingest; include/lc3plus_batch.h "Packet ingest"): the bits of item_status and the words of a stream's stats
ING_USED, ING_DUPLICATE, ING_LATE, ING_EARLY, ING_BAD_STREAM, ING_EMPTY, ING_REFUSED, ING_INVALID = 1, 2, 4, 8, 16, 32, 64, 128
ING_STATS_WORDS = 4
# packet egress (Batch.egress, DecBatch.egress, plan_egress; include/lc3plus_batch.h "Packet egress"): the bits of cell_status, of pkt_flags, the words of a route's stats
EGR_SENT, EGR_LOST, EGR_INVALID, EGR_SKIPPED, EGR_ABSENT, EGR_BAD_ROUTE, EGR_OVERFLOW = 1, 2, 4, 8, 16, 32, 64
EGR_PKT_OVERFLOW = 1
EGR_STATS_WORDS = 4
# RTP framing (DecBatch.rtp_parse, Batch.rtp_stamp, DecBatch.rtp_stamp, plan_rtp_parse, plan_rtp_stamp; include/lc3plus_batch.h "RTP framing"): an item's status
# (also its word in stats), the bits of pkt_status, the marker modes
(RTP_OK, RTP_RANGE, RTP_SHORT, RTP_VERSION, RTP_RTCP, RTP_HEADER, RTP_PADDING, RTP_PAYLOAD_ROOM, RTP_UNKNOWN_SSRC, RTP_PAYLOAD_TYPE) = range(10)
RTP_STATS_WORDS = 16
RTP_STAMPED, RTP_ST_BAD_ROUTE, RTP_ST_OVERFLOW, RTP_ST_RANGE = 1, 2, 4, 8
RTP_MARKER_NEVER, RTP_MARKER_AFTER_HOLE = 0, 1
# Reception reports (DecBatch.rtcp_stats, plan_rtcp_stats; include/lc3plus_batch.h "Reception reports"): the words of a stream's state, an item's status, the
# words of a stream's stats, a report block's bytes
(RR_FLAGS, RR_BASE_SEQ, RR_MAX_SEQ, RR_CYCLES, RR_BAD_SEQ, RR_RECEIVED, RR_EXPECTED_PRIOR, RR_RECEIVED_PRIOR, RR_TRANSIT, RR_JITTER) = range(10)
RR_STATE_WORDS = 10
RR_STARTED = 1
RR_DROPPED, RR_COUNTED, RR_JUMP, RR_RESTART, RR_REORDERED = range(5)
RR_ST_COUNTED, RR_ST_JUMP, RR_ST_RESTART, RR_ST_REORDERED = range(4)
RR_STATS_WORDS = 4
RR_BLOCK_BYTES = 24
RR_MAX_DROPOUT, RR_MAX_MISORDER = 3000, 100
# Secure RTP (srtp_make_context, Batch.srtp_protect_device, DecBatch.srtp_unprotect, plan_srtp_protect, plan_srtp_unprotect; include/lc3plus_batch.h "Secure
# RTP"): the words of a context, the bits of a protected packet's status, the words of a source's state, an item's status (also its word in stats)
SRTP_CTX_WORDS = 64
SRTP_PROTECTED, SRTP_NOT_STAMPED, SRTP_BAD_ROUTE, SRTP_RANGE, SRTP_OVERFLOW = 1, 2, 4, 8, 16
SRTP_STATE_WORDS = 8
SRTP_FLAGS, SRTP_ROC, SRTP_S_L, SRTP_WIN_LO, SRTP_WIN_HI = range(5)
SRTP_STARTED = 1
(SRTP_OK, SRTP_UN_RANGE, SRTP_SHORT, SRTP_VERSION, SRTP_RTCP, SRTP_HEADER, SRTP_UNKNOWN_SSRC, SRTP_REPLAY_OLD, SRTP_REPLAYED, SRTP_AUTH) = range(10)
SRTP_STATS_WORDS = 16
# Secure RTP, AEAD (srtp_gcm_make_context, Batch.srtp_gcm_protect_device, DecBatch.srtp_gcm_unprotect, plan_srtp_gcm_protect, plan_srtp_gcm_unprotect;
# include/lc3plus_batch.h "Secure RTP, AEAD"): the context's words and the tag's bytes; every other constant is SRTP_*'s
SRTP_GCM_CTX_WORDS = 128
SRTP_GCM_TAG_BYTES = 16
# Redundant audio (Batch.red_pack_device, DecBatch.red_pack_device, DecBatch.red_unpack, plan_red_pack, plan_red_unpack; include/lc3plus_batch.h "Redundant
# audio"): the deepest redundancy, the flag of a BAD packet, the words of a route's stats, an item's status (also its word in stats), the words of the dropped blocks
RED_MAX_DEPTH = 4
RED_PKT_BAD = 2
RED_STATS_WORDS = 4
(RED_OK, RED_DROPPED, RED_RANGE, RED_SHORT, RED_DEPTH, RED_LENGTH, RED_PAYLOAD_TYPE) = range(7)
RED_DROP_TYPE, RED_DROP_OFFSET, RED_DROP_EMPTY = 8, 9, 10
RED_UNPACK_STATS_WORDS = 16
# Generic FEC (Batch.fec_encode_device, DecBatch.fec_encode, DecBatch.fec_recover, plan_fec_encode, plan_fec_recover; include/lc3plus_batch.h "Generic FEC"): the
# largest group, the words of a route's state and of its stats, the flag of an EMPTY entry, an FEC item's status (also its word in stats)
FEC_MAX_GROUP = 16
FEC_STATE_WORDS = 8
FEC_ROUTE_STATS_WORDS = 4
FEC_PKT_EMPTY = 2
(FEC_RECOVERED, FEC_DROPPED, FEC_RANGE, FEC_SHORT, FEC_HEADER, FEC_LENGTH, FEC_COMPLETE, FEC_MISSING, FEC_PARTIAL, FEC_OVERFLOW) = range(10)
FEC_STATS_WORDS = 16
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
        L.lc3plus_dec_batch_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.lc3plus_frame_info_side.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.lc3plus_reject_name.argtypes = [C.c_int]; L.lc3plus_reject_name.restype = C.c_char_p
        L.lc3plus_dec_batch_ingest.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p, C.c_int]
        L.lc3plus_plan_ingest.argtypes = [C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 7 + [C.c_int, C.c_int] + [C.c_void_p] * 7
        egr = ([C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                C.c_void_p, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_void_p, C.c_void_p, C.c_int])
        L.lc3plus_enc_batch_egress.argtypes = [C.c_void_p] + egr
        L.lc3plus_dec_batch_egress.argtypes = [C.c_void_p] + egr
        L.lc3plus_plan_egress.argtypes = [C.c_int] + egr
        L.lc3plus_egress_work_bytes.argtypes = [C.c_int, C.c_int]; L.lc3plus_egress_work_bytes.restype = C.c_int64
        parse = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p, C.c_int]
        L.lc3plus_dec_batch_rtp_parse.argtypes = [C.c_void_p] + parse
        L.lc3plus_plan_rtp_parse.argtypes = [C.c_int] + parse
        L.lc3plus_rtp_sort_ssrc.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        stamp = ([C.c_int64] + [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
        L.lc3plus_enc_batch_rtp_stamp.argtypes = [C.c_void_p] + stamp
        L.lc3plus_dec_batch_rtp_stamp.argtypes = [C.c_void_p] + stamp
        L.lc3plus_plan_rtp_stamp.argtypes = stamp
        rr = [C.c_int64] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.lc3plus_dec_batch_rtcp_stats.argtypes = [C.c_void_p] + rr + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        L.lc3plus_plan_rtcp_stats.argtypes = rr
        L.lc3plus_rtcp_workspace_bytes.argtypes = [C.c_int64, C.c_int]; L.lc3plus_rtcp_workspace_bytes.restype = C.c_int64
        L.lc3plus_srtp_make_context.argtypes = [C.c_void_p] * 3
        prot = ([C.c_int64] + [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 4)
        L.lc3plus_enc_batch_srtp_protect.argtypes = [C.c_void_p] + prot + [C.c_void_p, C.c_int]
        L.lc3plus_dec_batch_srtp_protect.argtypes = [C.c_void_p] + prot + [C.c_void_p, C.c_int]
        L.lc3plus_plan_srtp_protect.argtypes = prot
        unp = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4
        L.lc3plus_dec_batch_srtp_unprotect.argtypes = [C.c_void_p] + unp + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        L.lc3plus_plan_srtp_unprotect.argtypes = unp
        L.lc3plus_srtp_workspace_bytes.argtypes = [C.c_int64, C.c_int]; L.lc3plus_srtp_workspace_bytes.restype = C.c_int64
        L.lc3plus_srtp_gcm_make_context.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        gprot, gunp = prot[:18] + prot[19:], unp[:10] + unp[11:]         # the AEAD calls: the same lists without tag_len
        L.lc3plus_enc_batch_srtp_gcm_protect.argtypes = [C.c_void_p] + gprot + [C.c_void_p, C.c_int]
        L.lc3plus_dec_batch_srtp_gcm_protect.argtypes = [C.c_void_p] + gprot + [C.c_void_p, C.c_int]
        L.lc3plus_plan_srtp_gcm_protect.argtypes = gprot
        L.lc3plus_dec_batch_srtp_gcm_unprotect.argtypes = [C.c_void_p] + gunp + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        L.lc3plus_plan_srtp_gcm_unprotect.argtypes = gunp
        red = ([C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                C.c_int] + [C.c_void_p] * 6 + [C.c_void_p, C.c_void_p, C.c_int])
        L.lc3plus_enc_batch_red_pack.argtypes = [C.c_void_p] + red
        L.lc3plus_dec_batch_red_pack.argtypes = [C.c_void_p] + red
        L.lc3plus_plan_red_pack.argtypes = [C.c_int] + red
        L.lc3plus_red_work_bytes.argtypes = [C.c_int64]; L.lc3plus_red_work_bytes.restype = C.c_int64
        unred = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p, C.c_int]
        L.lc3plus_dec_batch_red_unpack.argtypes = [C.c_void_p] + unred
        L.lc3plus_plan_red_unpack.argtypes = [C.c_int] + unred
        fec = ([C.c_int64] + [C.c_void_p] * 7 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                C.c_int64] + [C.c_void_p] * 10 + [C.c_void_p, C.c_void_p, C.c_int])
        L.lc3plus_enc_batch_fec_encode.argtypes = [C.c_void_p] + fec
        L.lc3plus_dec_batch_fec_encode.argtypes = [C.c_void_p] + fec
        L.lc3plus_plan_fec_encode.argtypes = fec
        L.lc3plus_fec_work_bytes.argtypes = [C.c_int, C.c_int]; L.lc3plus_fec_work_bytes.restype = C.c_int64
        L.lc3plus_fec_recover_work_bytes.argtypes = [C.c_int, C.c_int]; L.lc3plus_fec_recover_work_bytes.restype = C.c_int64
        unfec = ([C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 6 +
                 [C.c_void_p, C.c_int])
        L.lc3plus_dec_batch_fec_recover.argtypes = [C.c_void_p] + unfec
        L.lc3plus_plan_fec_recover.argtypes = [C.c_int] + unfec
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


EGR_OPTIONAL = ("pkt_flags", "wire_total", "next_seq", "stats", "cell_status")
EGR_OUTPUTS = ("pkt_route", "pkt_seq", "pkt_frame", "pkt_offset", "pkt_size", "pkt_flags", "n_packets", "wire_total", "next_seq", "stats", "cell_status")


def egress_work_bytes(n_routes, n_frames):
    """bytes of the workspace of an egress call (lc3plus_egress_work_bytes); 0 for a shape the calls refuse"""
    return int(load_library().lc3plus_egress_work_bytes(int(n_routes), int(n_frames)))


def _egress_arrays(n_streams, frames, offsets, num_bytes, seq_base, flags, counts, route_src, wire, optional):
    """the arrays of an egress call as the C calls take them: (inputs by name, None for a NULL one; outputs in EGR_OUTPUTS order likewise; work)"""
    frames = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32)
    if offsets.ndim != 2 or offsets.shape != num_bytes.shape or offsets.shape[0] != n_streams:
        raise ValueError("offsets and num_bytes must have shape [n_streams, n_frames]")
    T = offsets.shape[1]
    seq_base = (np.asarray(seq_base).astype(np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)       # 0 ... 2^32 - 1 and negative values both fit
    R = seq_base.size
    if flags is not None:
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        if flags.shape != offsets.shape:
            raise ValueError("flags must have the shape of offsets")
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if counts.size != n_streams:
            raise ValueError("counts holds one entry per stream")
    if route_src is not None:
        route_src = np.ascontiguousarray(route_src, dtype=np.int32).reshape(-1)
        if route_src.size != R:
            raise ValueError("route_src and seq_base hold one entry per route")
    if wire is not None:
        wire = np.array(wire, dtype=np.uint8).reshape(-1)             # a copy: the call's wire buffer starts with these contents
    n = R * T
    ins = dict(frames=frames, offsets=offsets, num_bytes=num_bytes, flags=flags, counts=counts, route_src=route_src, seq_base=seq_base, wire=wire)
    outs = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32),
            np.zeros(n, np.uint8) if "pkt_flags" in optional else None, np.zeros(1, np.int64), np.zeros(1, np.int64) if "wire_total" in optional else None,
            np.zeros(R, np.int32) if "next_seq" in optional else None, np.zeros((R, EGR_STATS_WORDS), np.int32) if "stats" in optional else None,
            np.zeros((R, T), np.uint8) if "cell_status" in optional else None]
    work = np.zeros(max(egress_work_bytes(R, T), 8) // 8, np.int64)
    return ins, outs, work


def _egress_result(ins, outs):
    r = dict(zip(EGR_OUTPUTS, outs))
    r["n_packets"] = int(r["n_packets"][0])
    r["wire_total"] = int(r["wire_total"][0]) if r["wire_total"] is not None else None
    r["wire"] = ins["wire"]
    return r


def plan_egress(n_streams, frames, offsets, num_bytes, seq_base, max_frame_bytes, flags=None, skip_mask=0, counts=None, route_src=None, seq_bits=16,
                order=PACK_STREAM_MAJOR, wire=None, wire_capacity=None, header_room=0, align=1, optional=EGR_OPTIONAL, frames_capacity=None):
    """The rule of Batch.egress / DecBatch.egress on the host (lc3plus_plan_egress, no device needed): frames (uint8, frames_capacity bytes of it: all by
    default), offsets (int64) / num_bytes [n_streams, n_frames], seq_base [n_routes]; optional flags [n_streams, n_frames] with skip_mask, counts [n_streams],
    route_src [n_routes]; wire: None (in place) or the wire buffer's contents before the call (uint8; wire_capacity bytes of it: all by default).
    -> dict of the list arrays pkt_route, pkt_seq, pkt_frame, pkt_offset (int64), pkt_size, pkt_flags (uint8) [n_routes * n_frames] (zero behind n_packets),
    n_packets, wire_total (ints), next_seq [n_routes], stats [n_routes, EGR_STATS_WORDS], cell_status [n_routes, n_frames] (uint8) and wire (the buffer after
    the call, or None); the outputs of EGR_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call
    refuses."""
    ins, outs, work = _egress_arrays(n_streams, frames, offsets, num_bytes, seq_base, flags, counts, route_src, wire, optional)
    ptr = lambda a: a.ctypes.data if a is not None else None
    fcap = ins["frames"].size if frames_capacity is None else int(frames_capacity)
    wcap = (ins["wire"].size if ins["wire"] is not None else 0) if wire_capacity is None else int(wire_capacity)
    pad = np.zeros(8, np.uint8)                                       # an empty array still has to be a pointer
    rc = load_library().lc3plus_plan_egress(
        int(n_streams), ins["offsets"].shape[1], ptr(ins["frames"] if ins["frames"].size else pad), fcap, ptr(ins["offsets"]), ptr(ins["num_bytes"]),
        int(max_frame_bytes), ptr(ins["flags"]), int(skip_mask), ptr(ins["counts"]), ins["seq_base"].size, ptr(ins["route_src"]), ptr(ins["seq_base"]),
        int(seq_bits), int(order), ptr(ins["wire"]), wcap, int(header_room), int(align), *[ptr(a) for a in outs], ptr(work), None, 0)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_egress")
    return _egress_result(ins, outs)


class _Egress:
    """Packet egress of both batch kinds (lc3plus_{enc,dec}_batch_egress; include/lc3plus_batch.h "Packet egress")."""

    def egress_device(self, n_frames, d_frames_ptr, frames_capacity, d_offsets_ptr, d_num_bytes_ptr, max_frame_bytes, n_routes, d_seq_base_ptr, d_pkt_route_ptr,
                      d_pkt_seq_ptr, d_pkt_frame_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, d_n_packets_ptr, d_work_ptr, d_flags_ptr=None, skip_mask=0,
                      d_counts_ptr=None, d_route_src_ptr=None, seq_bits=16, order=PACK_STREAM_MAJOR, d_wire_ptr=None, wire_capacity=0, header_room=0, align=1,
                      d_pkt_flags_ptr=None, d_wire_total_ptr=None, d_next_seq_ptr=None, d_stats_ptr=None, d_cell_status_ptr=None, hip_stream=None, sync=False):
        """Raw device pointers only - the tables offsets (int64), num_bytes, optional flags [n_streams, n_frames] and counts [n_streams] of the frames in `frames`,
        the routes seq_base and optional route_src [n_routes] -> the packet list pkt_* [n_routes * n_frames], n_packets and the optional wire_total (one int64
        each), next_seq [n_routes], stats [n_routes, EGR_STATS_WORDS], cell_status [n_routes, n_frames]; with d_wire_ptr the frames are copied there behind
        header_room bytes each.  work: egress_work_bytes(n_routes, n_frames) bytes.  Stateless: nothing of the batch's streams is read or written.  Queued on
        hip_stream; returns at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self._ssf("_egress")(self.h, int(n_frames), p(d_frames_ptr), int(frames_capacity), p(d_offsets_ptr), p(d_num_bytes_ptr), int(max_frame_bytes),
                                  p(d_flags_ptr), int(skip_mask), p(d_counts_ptr), int(n_routes), p(d_route_src_ptr), p(d_seq_base_ptr), int(seq_bits), int(order),
                                  p(d_wire_ptr), int(wire_capacity), int(header_room), int(align), p(d_pkt_route_ptr), p(d_pkt_seq_ptr), p(d_pkt_frame_ptr),
                                  p(d_pkt_offset_ptr), p(d_pkt_size_ptr), p(d_pkt_flags_ptr), p(d_n_packets_ptr), p(d_wire_total_ptr), p(d_next_seq_ptr),
                                  p(d_stats_ptr), p(d_cell_status_ptr), p(d_work_ptr), p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, self._ss + "_egress")

    def egress(self, frames, offsets, num_bytes, seq_base, max_frame_bytes, flags=None, skip_mask=0, counts=None, route_src=None, seq_bits=16,
               order=PACK_STREAM_MAJOR, wire=None, wire_capacity=None, header_room=0, align=1, optional=EGR_OPTIONAL, frames_capacity=None):
        """Host convenience: the arrays of plan_egress uploaded, the egress run on the device and downloaded -> the dict plan_egress gives.  Device memory through
        the HIP runtime (hipMalloc / hipMemcpy on the current device: the batch's, unless the caller has switched), freed before it returns."""
        ins, outs, work = _egress_arrays(self.n_streams, frames, offsets, num_bytes, seq_base, flags, counts, route_src, wire, optional)
        fcap = ins["frames"].size if frames_capacity is None else int(frames_capacity)
        wcap = (ins["wire"].size if ins["wire"] is not None else 0) if wire_capacity is None else int(wire_capacity)
        hip = C.CDLL("libamdhip64.so")
        names = ("frames", "offsets", "num_bytes", "flags", "counts", "route_src", "seq_base", "wire")
        arrays = [ins[k] for k in names] + outs + [work]
        ptrs = []
        try:
            for a in arrays:
                d = C.c_void_p()                                    # stays NULL for an argument that is None
                ptrs.append(d)
                if a is None:
                    continue
                if hip.hipMalloc(C.byref(d), C.c_size_t(max(a.nbytes, 8))) != 0:
                    raise LC3Error(1, "hipMalloc")
                if a.nbytes and hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1)) != 0:
                    raise LC3Error(1, "hipMemcpy")
            v = dict(zip(names + EGR_OUTPUTS + ("work",), [d.value for d in ptrs]))
            self.egress_device(ins["offsets"].shape[1], v["frames"], fcap, v["offsets"], v["num_bytes"], max_frame_bytes, ins["seq_base"].size, v["seq_base"],
                               v["pkt_route"], v["pkt_seq"], v["pkt_frame"], v["pkt_offset"], v["pkt_size"], v["n_packets"], v["work"], v["flags"], skip_mask,
                               v["counts"], v["route_src"], seq_bits, order, v["wire"], wcap, header_room, align, v["pkt_flags"], v["wire_total"], v["next_seq"],
                               v["stats"], v["cell_status"], sync=True)
            for a, d in zip([ins["wire"]] + outs, ptrs[7:8] + ptrs[8:8 + len(outs)]):
                if a is not None and a.nbytes and hip.hipMemcpy(C.c_void_p(a.ctypes.data), d, C.c_size_t(a.nbytes), C.c_int(2)) != 0:
                    raise LC3Error(1, "hipMemcpy")
        finally:
            for d in ptrs:
                if d.value:
                    hip.hipFree(d)
        return _egress_result(ins, outs)


def _u32(x):
    """32-bit words however they are given: 0 ... 2^32 - 1 and negative values both fit"""
    return (np.asarray(x).astype(np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


@contextlib.contextmanager
def _on_device(arrays):
    """the arrays (None: a NULL pointer) in device memory through the HIP runtime (hipMalloc / hipMemcpy on the current device) -> (their pointers, a function
    that copies a device array back into its host array); everything is freed at the end"""
    hip = C.CDLL("libamdhip64.so")
    ptrs = []

    def back(k):
        a = arrays[k]
        if a is not None and a.nbytes and hip.hipMemcpy(C.c_void_p(a.ctypes.data), ptrs[k], C.c_size_t(a.nbytes), C.c_int(2)) != 0:
            raise LC3Error(1, "hipMemcpy")
    try:
        for a in arrays:
            d = C.c_void_p()                                        # stays NULL for an argument that is None
            ptrs.append(d)
            if a is None:
                continue
            if hip.hipMalloc(C.byref(d), C.c_size_t(max(a.nbytes, 8))) != 0:
                raise LC3Error(1, "hipMalloc")
            if a.nbytes and hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1)) != 0:
                raise LC3Error(1, "hipMemcpy")
        yield [d.value for d in ptrs], back
    finally:
        for d in ptrs:
            if d.value:
                hip.hipFree(d)


RTP_PARSE_OPTIONAL = ("timestamp", "marker", "status", "stats")
RTP_PARSE_OUTPUTS = ("stream", "seq", "offsets", "num_bytes", "timestamp", "marker", "status", "stats")
RTP_STAMP_OPTIONAL = ("pkt_status", "next_ts", "next_resume")


def rtp_sort_ssrc(ssrc_key, ssrc_stream):
    """An SSRC table in the order rtp_parse needs (lc3plus_rtp_sort_ssrc): -> (keys ascending as uint32, as int32 words; each key's stream).  LC3Error for an
    empty table and for a key that occurs twice."""
    key, stream = _u32(ssrc_key).copy(), np.array(ssrc_stream, dtype=np.int32).reshape(-1)
    if key.size != stream.size:
        raise ValueError("ssrc_key and ssrc_stream hold one entry per sender")
    rc = load_library().lc3plus_rtp_sort_ssrc(key.size, key.ctypes.data if key.size else None, stream.ctypes.data if stream.size else None)
    if rc:
        raise LC3Error(rc, "lc3plus_rtp_sort_ssrc")
    return key, stream


def _rtp_parse_arrays(n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type, optional):
    """the arrays of a parse call as the C calls take them: (inputs ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type - None for NULL; outputs in
    RTP_PARSE_OUTPUTS order likewise)"""
    ring = np.ascontiguousarray(ring, dtype=np.uint8).reshape(-1)
    dg_offsets = np.ascontiguousarray(dg_offsets, dtype=np.int64).reshape(-1)
    dg_sizes = np.ascontiguousarray(dg_sizes, dtype=np.int32).reshape(-1)
    key, stream = _u32(ssrc_key), np.ascontiguousarray(ssrc_stream, dtype=np.int32).reshape(-1)
    if dg_offsets.size != dg_sizes.size or key.size != stream.size:
        raise ValueError("dg_offsets and dg_sizes hold one entry per datagram, ssrc_key and ssrc_stream one per sender")
    if payload_type is not None:
        payload_type = np.ascontiguousarray(payload_type, dtype=np.int32).reshape(-1)
        if payload_type.size != n_streams:
            raise ValueError("payload_type holds one entry per stream")
    n = dg_offsets.size
    outs = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32),
            np.zeros(n, np.int32) if "timestamp" in optional else None, np.zeros(n, np.uint8) if "marker" in optional else None,
            np.zeros(n, np.uint8) if "status" in optional else None, np.zeros(RTP_STATS_WORDS, np.int32) if "stats" in optional else None]
    return [ring, dg_offsets, dg_sizes, key, stream, payload_type], outs


def plan_rtp_parse(n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type=None, payload_room=0, optional=RTP_PARSE_OPTIONAL,
                   ring_capacity=None):
    """The rule of DecBatch.rtp_parse on the host (lc3plus_plan_rtp_parse, no device needed): ring (uint8, ring_capacity bytes of it: all by default), the
    datagrams dg_offsets (int64) / dg_sizes [n], the senders ssrc_key (ascending as uint32: rtp_sort_ssrc) / ssrc_stream, optional payload_type [n_streams]
    -> dict of stream, seq, offsets (int64), num_bytes [n] - the item arrays of ingest and probe - and timestamp [n], marker, status (uint8) [n] and stats
    [RTP_STATS_WORDS]; those of RTP_PARSE_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call
    refuses."""
    ins, outs = _rtp_parse_arrays(n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type, optional)
    pad = np.zeros(8, np.uint8)                                       # an empty array still has to be a pointer
    ptr = lambda a: (a if a.size else pad).ctypes.data if a is not None else None
    cap = ins[0].size if ring_capacity is None else int(ring_capacity)
    rc = load_library().lc3plus_plan_rtp_parse(int(n_streams), ins[1].size, ptr(ins[0]), cap, ptr(ins[1]), ptr(ins[2]), ins[3].size, ptr(ins[3]), ptr(ins[4]),
                                               ptr(ins[5]), int(payload_room), *[ptr(a) for a in outs], None, 0)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_rtp_parse")
    return dict(zip(RTP_PARSE_OUTPUTS, outs))


def _rtp_stamp_arrays(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, pkt_flags, n_packets, ssrc, ts_base, payload_type, n_frames, cell_status, resume,
                      route_stats, wire, optional):
    """the arrays of a stamp call as the C calls take them: (inputs in the header's order, None for NULL; wire, a copy; outputs pkt_status, next_ts,
    next_resume likewise)"""
    route = np.ascontiguousarray(pkt_route, dtype=np.int32).reshape(-1)
    m = route.size
    seq, frame = _u32(pkt_seq), np.ascontiguousarray(pkt_frame, dtype=np.int32).reshape(-1)
    off, size = np.ascontiguousarray(pkt_offset, dtype=np.int64).reshape(-1), np.ascontiguousarray(pkt_size, dtype=np.int32).reshape(-1)
    if not (seq.size == frame.size == off.size == size.size == m):
        raise ValueError("the list arrays hold one entry per packet")
    flags = np.ascontiguousarray(pkt_flags, dtype=np.uint8).reshape(-1) if pkt_flags is not None else None
    if flags is not None and flags.size != m:
        raise ValueError("pkt_flags holds one entry per packet")
    ssrc, ts_base, payload_type = _u32(ssrc), _u32(ts_base), np.ascontiguousarray(payload_type, dtype=np.int32).reshape(-1)
    R = ssrc.size
    if ts_base.size != R or payload_type.size != R:
        raise ValueError("ssrc, ts_base and payload_type hold one entry per route")
    if cell_status is not None:
        cell_status = np.ascontiguousarray(cell_status, dtype=np.uint8)
        if cell_status.shape != (R, int(n_frames)):
            raise ValueError("cell_status must have shape [n_routes, n_frames]")
    if resume is not None:
        resume = np.ascontiguousarray(resume, dtype=np.uint8).reshape(-1)
        if resume.size != R:
            raise ValueError("resume holds one entry per route")
    if route_stats is not None:
        route_stats = np.ascontiguousarray(route_stats, dtype=np.int32)
        if route_stats.shape != (R, EGR_STATS_WORDS):
            raise ValueError("route_stats must have shape [n_routes, EGR_STATS_WORDS]")
    count = np.array([m if n_packets is None else int(n_packets)], np.int64)
    wire = np.array(wire, dtype=np.uint8).reshape(-1)                 # a copy: the call's wire buffer starts with these contents
    outs = [np.zeros(m, np.uint8) if "pkt_status" in optional else None, np.zeros(R, np.int32) if "next_ts" in optional else None,
            np.zeros(R, np.uint8) if "next_resume" in optional else None]
    return [count, route, seq, frame, off, size, flags, ssrc, ts_base, payload_type, cell_status, resume, route_stats], wire, outs


def plan_rtp_stamp(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type, ts_step, n_frames, wire, header_room=12, payload_room=0,
                   pkt_flags=None, n_packets=None, marker_mode=RTP_MARKER_NEVER, cell_status=None, resume=None, route_stats=None, wire_capacity=None,
                   optional=RTP_STAMP_OPTIONAL):
    """The rule of Batch.rtp_stamp / DecBatch.rtp_stamp on the host (lc3plus_plan_rtp_stamp, no device needed): the egress's packet list pkt_* [max_packets]
    (n_packets of it: all by default), per route ssrc, ts_base, payload_type [n_routes], optional cell_status [n_routes, n_frames], resume [n_routes] and
    route_stats [n_routes, EGR_STATS_WORDS] (the egress's stats); wire: the wire buffer's contents before the call (uint8; wire_capacity bytes of it: all by
    default) -> dict of wire (the buffer after the call), pkt_status (uint8) [max_packets] (zero behind n_packets), next_ts [n_routes] and next_resume (uint8)
    [n_routes]; those of RTP_STAMP_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    ins, wire, outs = _rtp_stamp_arrays(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, pkt_flags, n_packets, ssrc, ts_base, payload_type, n_frames,
                                        cell_status, resume, route_stats, wire, optional)
    pad = np.zeros(8, np.uint8)
    ptr = lambda a: (a if a.size else pad).ctypes.data if a is not None else None
    wcap = wire.size if wire_capacity is None else int(wire_capacity)
    rc = load_library().lc3plus_plan_rtp_stamp(ins[1].size, *[ptr(a) for a in ins[:7]], ins[7].size, int(n_frames), ptr(ins[7]), ptr(ins[8]), ptr(ins[9]),
                                               int(ts_step), int(marker_mode), ptr(ins[10]), ptr(ins[11]), ptr(ins[12]), ptr(wire), wcap, int(header_room),
                                               int(payload_room), *[ptr(a) for a in outs], None, 0)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_rtp_stamp")
    return dict(zip(RTP_STAMP_OPTIONAL, outs), wire=wire)


class _RtpStamp:
    """The send side of the RTP framing for both batch kinds (lc3plus_{enc,dec}_batch_rtp_stamp; include/lc3plus_batch.h "RTP framing")."""

    def rtp_stamp_device(self, max_packets, d_n_packets_ptr, d_pkt_route_ptr, d_pkt_seq_ptr, d_pkt_frame_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, n_routes, n_frames,
                         d_ssrc_ptr, d_ts_base_ptr, d_payload_type_ptr, ts_step, d_wire_ptr, wire_capacity, header_room=12, payload_room=0, d_pkt_flags_ptr=None,
                         marker_mode=RTP_MARKER_NEVER, d_cell_status_ptr=None, d_resume_ptr=None, d_route_stats_ptr=None, d_pkt_status_ptr=None,
                         d_next_ts_ptr=None, d_next_resume_ptr=None, hip_stream=None, sync=False):
        """Raw device pointers only - the egress's packet list pkt_* [max_packets] with its length n_packets (one int64, read when the kernel runs), per route
        ssrc, ts_base, payload_type [n_routes] and the optional cell_status [n_routes, n_frames], resume [n_routes] (uint8) and route_stats (the egress's
        stats) -> an RTP header in the header room of every packet of the egress's wire buffer, payload_room bytes in front of the frame, and the optional
        pkt_status [max_packets] (uint8), next_ts [n_routes], next_resume [n_routes] (uint8).  Stateless: nothing of the batch's streams is read or written.
        Queued on hip_stream; returns at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self._ssf("_rtp_stamp")(self.h, int(max_packets), p(d_n_packets_ptr), p(d_pkt_route_ptr), p(d_pkt_seq_ptr), p(d_pkt_frame_ptr), p(d_pkt_offset_ptr),
                                     p(d_pkt_size_ptr), p(d_pkt_flags_ptr), int(n_routes), int(n_frames), p(d_ssrc_ptr), p(d_ts_base_ptr), p(d_payload_type_ptr),
                                     int(ts_step), int(marker_mode), p(d_cell_status_ptr), p(d_resume_ptr), p(d_route_stats_ptr), p(d_wire_ptr), int(wire_capacity),
                                     int(header_room), int(payload_room), p(d_pkt_status_ptr), p(d_next_ts_ptr), p(d_next_resume_ptr), p(hip_stream),
                                     1 if sync else 0)
        if rc:
            raise LC3Error(rc, self._ss + "_rtp_stamp")

    def rtp_stamp(self, pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type, ts_step, n_frames, wire, header_room=12, payload_room=0,
                  pkt_flags=None, n_packets=None, marker_mode=RTP_MARKER_NEVER, cell_status=None, resume=None, route_stats=None, wire_capacity=None,
                  optional=RTP_STAMP_OPTIONAL):
        """Host convenience: the arrays of plan_rtp_stamp uploaded, stamped on the device and downloaded -> the dict plan_rtp_stamp gives.  Device memory through
        the HIP runtime (on the current device: the batch's, unless the caller has switched), freed before it returns."""
        ins, wire, outs = _rtp_stamp_arrays(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, pkt_flags, n_packets, ssrc, ts_base, payload_type, n_frames,
                                            cell_status, resume, route_stats, wire, optional)
        wcap = wire.size if wire_capacity is None else int(wire_capacity)
        arrays = ins + [wire] + outs
        with _on_device(arrays) as (v, back):
            self.rtp_stamp_device(ins[1].size, v[0], v[1], v[2], v[3], v[4], v[5], ins[7].size, n_frames, v[7], v[8], v[9], ts_step, v[13], wcap, header_room,
                                  payload_room, v[6], marker_mode, v[10], v[11], v[12], v[14], v[15], v[16], sync=True)
            for k in range(13, 17):
                back(k)
        return dict(zip(RTP_STAMP_OPTIONAL, outs), wire=wire)


RED_PACK_OPTIONAL = ("red_flags", "red_blocks", "wire_total", "route_stats", "tail")
RED_PACK_OUTPUTS = ("red_offset", "red_size", "red_flags", "red_blocks", "wire_total", "route_stats")
RED_UNPACK_OPTIONAL = ("timestamp", "gen", "status", "stats")
RED_UNPACK_OUTPUTS = ("stream", "seq", "offsets", "num_bytes", "timestamp", "gen", "status", "stats")


def red_work_bytes(max_packets):
    """bytes of the workspace of a red_pack call (lc3plus_red_work_bytes); 0 for a max_packets the calls refuse"""
    return int(load_library().lc3plus_red_work_bytes(int(max_packets)))


def red_tail_stride(max_frame_bytes):
    """the smallest tail_stride a red_pack call takes for frames of up to max_frame_bytes bytes"""
    return (min(int(max_frame_bytes), 1023) + 15) & ~15


def _red_pack_arrays(n_streams, frames, offsets, num_bytes, pkt_route, pkt_frame, n_packets, block_pt, max_depth, depth, flags, counts, route_src, tail_bytes, tail_sizes,
                     tail_stride, wire, optional):
    """the arrays of a pack call as the C calls take them: (inputs by name, None for a NULL one; outputs in RED_PACK_OUTPUTS order, then tail_bytes and tail_sizes;
    work)"""
    frames = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32)
    if offsets.ndim != 2 or offsets.shape != num_bytes.shape or offsets.shape[0] != n_streams:
        raise ValueError("offsets and num_bytes must have shape [n_streams, n_frames]")
    route = np.ascontiguousarray(pkt_route, dtype=np.int32).reshape(-1)
    frame = np.ascontiguousarray(pkt_frame, dtype=np.int32).reshape(-1)
    if route.size != frame.size:
        raise ValueError("pkt_route and pkt_frame hold one entry per packet")
    m = route.size
    block_pt = np.ascontiguousarray(block_pt, dtype=np.int32).reshape(-1)
    R, D = block_pt.size, int(max_depth)
    opt = lambda a, dt, shape, what: None if a is None else _shaped(np.ascontiguousarray(a, dtype=dt), shape, what)
    flags = opt(flags, np.uint8, offsets.shape, "flags must have the shape of offsets")
    counts = opt(counts, np.int32, (n_streams,), "counts holds one entry per stream")
    route_src = opt(route_src, np.int32, (R,), "route_src and block_pt hold one entry per route")
    depth = opt(depth, np.int32, (R,), "depth holds one entry per route")
    if (tail_bytes is None) != (tail_sizes is None):
        raise ValueError("tail_bytes and tail_sizes come together")
    tail_bytes = opt(tail_bytes, np.uint8, (n_streams, D, int(tail_stride)), "tail_bytes must have shape [n_streams, max_depth, tail_stride]")
    tail_sizes = opt(tail_sizes, np.int32, (n_streams, D), "tail_sizes must have shape [n_streams, max_depth]")
    count = np.array([m if n_packets is None else int(n_packets)], np.int64)
    wire = np.array(wire, dtype=np.uint8).reshape(-1)                 # a copy: the call's wire buffer starts with these contents
    ins = dict(frames=frames, offsets=offsets, num_bytes=num_bytes, flags=flags, counts=counts, route_src=route_src, n_packets=count, pkt_route=route, pkt_frame=frame,
               depth=depth, block_pt=block_pt, tail_bytes=tail_bytes, tail_sizes=tail_sizes, wire=wire)
    tail = "tail" in optional
    outs = [np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, np.uint8) if "red_flags" in optional else None,
            np.zeros(m, np.uint8) if "red_blocks" in optional else None, np.zeros(1, np.int64) if "wire_total" in optional else None,
            np.zeros((R, RED_STATS_WORDS), np.int32) if "route_stats" in optional else None,
            np.zeros((n_streams, D, int(tail_stride)), np.uint8) if tail else None, np.zeros((n_streams, D), np.int32) if tail else None]
    work = np.zeros(max(red_work_bytes(max(m, 1)), 8) // 8, np.int64)
    return ins, outs, work


def _shaped(a, shape, what):
    if a.shape != tuple(shape):
        raise ValueError(what)
    return a


def _red_pack_result(ins, outs):
    r = dict(zip(RED_PACK_OUTPUTS + ("tail_bytes", "tail_sizes"), outs))
    r["wire_total"] = int(r["wire_total"][0]) if r["wire_total"] is not None else None
    r["wire"] = ins["wire"]
    return r


RED_PACK_INPUTS = ("frames", "offsets", "num_bytes", "flags", "counts", "route_src", "n_packets", "pkt_route", "pkt_frame", "depth", "block_pt", "tail_bytes", "tail_sizes",
                   "wire")


def plan_red_pack(n_streams, frames, offsets, num_bytes, max_frame_bytes, pkt_route, pkt_frame, block_pt, ts_step, wire, max_depth=1, depth=None,
                  max_packet_bytes=1 << 30, n_packets=None, flags=None, skip_mask=0, counts=None, route_src=None, tail_bytes=None, tail_sizes=None, tail_stride=None,
                  wire_capacity=None, header_room=12, align=1, optional=RED_PACK_OPTIONAL, frames_capacity=None):
    """The rule of Batch.red_pack_device / DecBatch.red_pack_device on the host (lc3plus_plan_red_pack, no device needed): the egress's frame tables - frames (uint8),
    offsets (int64) / num_bytes [n_streams, n_frames], optional flags with skip_mask, counts [n_streams], route_src [n_routes] - its in-place list pkt_route,
    pkt_frame [max_packets] (n_packets of it: all by default), block_pt [n_routes], optional depth [n_routes], the previous call's tail_bytes
    [n_streams, max_depth, tail_stride] / tail_sizes [n_streams, max_depth] (tail_stride: red_tail_stride(max_frame_bytes) by default) and wire, the wire buffer's
    contents before the call -> dict of red_offset (int64), red_size, red_flags, red_blocks (uint8) [max_packets] (zero behind n_packets), wire_total (int),
    route_stats [n_routes, RED_STATS_WORDS], tail_bytes / tail_sizes for the next call and wire (the buffer after the call); the outputs of RED_PACK_OPTIONAL
    not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    stride = red_tail_stride(max_frame_bytes) if tail_stride is None else int(tail_stride)
    ins, outs, work = _red_pack_arrays(n_streams, frames, offsets, num_bytes, pkt_route, pkt_frame, n_packets, block_pt, max_depth, depth, flags, counts, route_src,
                                       tail_bytes, tail_sizes, stride, wire, optional)
    pad = np.zeros(8, np.uint8)                                       # an empty array still has to be a pointer
    ptr = lambda a: (a if a.size else pad).ctypes.data if a is not None else None
    fcap = ins["frames"].size if frames_capacity is None else int(frames_capacity)
    wcap = ins["wire"].size if wire_capacity is None else int(wire_capacity)
    rc = load_library().lc3plus_plan_red_pack(
        int(n_streams), ins["offsets"].shape[1], ptr(ins["frames"]), fcap, ptr(ins["offsets"]), ptr(ins["num_bytes"]), int(max_frame_bytes), ptr(ins["flags"]),
        int(skip_mask), ptr(ins["counts"]), ins["block_pt"].size, ptr(ins["route_src"]), ins["pkt_route"].size, ptr(ins["n_packets"]), ptr(ins["pkt_route"]),
        ptr(ins["pkt_frame"]), int(max_depth), ptr(ins["depth"]), ptr(ins["block_pt"]), int(ts_step), int(max_packet_bytes), ptr(ins["tail_bytes"]),
        ptr(ins["tail_sizes"]), stride, ptr(outs[6]), ptr(outs[7]), ptr(ins["wire"]), wcap, int(header_room), int(align), *[ptr(a) for a in outs[:6]], ptr(work), None, 0)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_red_pack")
    return _red_pack_result(ins, outs)


class _RedPack:
    """The send side of the redundant audio for both batch kinds (lc3plus_{enc,dec}_batch_red_pack; include/lc3plus_batch.h "Redundant audio")."""

    def red_pack_device(self, n_frames, d_frames_ptr, frames_capacity, d_offsets_ptr, d_num_bytes_ptr, max_frame_bytes, n_routes, max_packets, d_n_packets_ptr,
                        d_pkt_route_ptr, d_pkt_frame_ptr, max_depth, d_block_pt_ptr, ts_step, max_packet_bytes, d_wire_ptr, wire_capacity, d_red_offset_ptr,
                        d_red_size_ptr, d_work_ptr, header_room=12, align=1, d_flags_ptr=None, skip_mask=0, d_counts_ptr=None, d_route_src_ptr=None, d_depth_ptr=None,
                        d_tail_bytes_in_ptr=None, d_tail_sizes_in_ptr=None, tail_stride=0, d_tail_bytes_out_ptr=None, d_tail_sizes_out_ptr=None, d_red_flags_ptr=None,
                        d_red_blocks_ptr=None, d_wire_total_ptr=None, d_route_stats_ptr=None, hip_stream=None, sync=False):
        """Raw device pointers only - the frame tables an egress call took, its in-place list pkt_route / pkt_frame [max_packets] with its length n_packets (one
        int64, read when the kernels run), block_pt [n_routes] and the optional depth [n_routes] and tails -> RFC 2198 payloads behind header_room bytes each in
        the wire buffer, the records red_offset (int64), red_size [max_packets] and the optional red_flags, red_blocks (uint8), wire_total (one int64),
        route_stats [n_routes, RED_STATS_WORDS] and the tails for the next call.  work: red_work_bytes(max_packets) bytes.  Stateless: nothing of the batch's
        streams is read or written.  Queued on hip_stream; returns at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self._ssf("_red_pack")(self.h, int(n_frames), p(d_frames_ptr), int(frames_capacity), p(d_offsets_ptr), p(d_num_bytes_ptr), int(max_frame_bytes),
                                    p(d_flags_ptr), int(skip_mask), p(d_counts_ptr), int(n_routes), p(d_route_src_ptr), int(max_packets), p(d_n_packets_ptr),
                                    p(d_pkt_route_ptr), p(d_pkt_frame_ptr), int(max_depth), p(d_depth_ptr), p(d_block_pt_ptr), int(ts_step), int(max_packet_bytes),
                                    p(d_tail_bytes_in_ptr), p(d_tail_sizes_in_ptr), int(tail_stride), p(d_tail_bytes_out_ptr), p(d_tail_sizes_out_ptr), p(d_wire_ptr),
                                    int(wire_capacity), int(header_room), int(align), p(d_red_offset_ptr), p(d_red_size_ptr), p(d_red_flags_ptr), p(d_red_blocks_ptr),
                                    p(d_wire_total_ptr), p(d_route_stats_ptr), p(d_work_ptr), p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, self._ss + "_red_pack")

    def red_pack(self, frames, offsets, num_bytes, max_frame_bytes, pkt_route, pkt_frame, block_pt, ts_step, wire, max_depth=1, depth=None, max_packet_bytes=1 << 30,
                 n_packets=None, flags=None, skip_mask=0, counts=None, route_src=None, tail_bytes=None, tail_sizes=None, tail_stride=None, wire_capacity=None,
                 header_room=12, align=1, optional=RED_PACK_OPTIONAL, frames_capacity=None):
        """Host convenience: the arrays of plan_red_pack uploaded, packed on the device and downloaded -> the dict plan_red_pack gives.  Device memory through the
        HIP runtime (on the current device: the batch's, unless the caller has switched), freed before it returns."""
        stride = red_tail_stride(max_frame_bytes) if tail_stride is None else int(tail_stride)
        ins, outs, work = _red_pack_arrays(self.n_streams, frames, offsets, num_bytes, pkt_route, pkt_frame, n_packets, block_pt, max_depth, depth, flags, counts,
                                           route_src, tail_bytes, tail_sizes, stride, wire, optional)
        fcap = ins["frames"].size if frames_capacity is None else int(frames_capacity)
        wcap = ins["wire"].size if wire_capacity is None else int(wire_capacity)
        arrays = [ins[k] for k in RED_PACK_INPUTS] + outs + [work]
        with _on_device(arrays) as (ptrs, back):
            v = dict(zip(RED_PACK_INPUTS + RED_PACK_OUTPUTS + ("tail_bytes_out", "tail_sizes_out", "work"), ptrs))
            self.red_pack_device(ins["offsets"].shape[1], v["frames"], fcap, v["offsets"], v["num_bytes"], max_frame_bytes, ins["block_pt"].size, ins["pkt_route"].size,
                                 v["n_packets"], v["pkt_route"], v["pkt_frame"], max_depth, v["block_pt"], ts_step, max_packet_bytes, v["wire"], wcap, v["red_offset"],
                                 v["red_size"], v["work"], header_room, align, v["flags"], skip_mask, v["counts"], v["route_src"], v["depth"], v["tail_bytes"],
                                 v["tail_sizes"], stride, v["tail_bytes_out"], v["tail_sizes_out"], v["red_flags"], v["red_blocks"], v["wire_total"], v["route_stats"],
                                 sync=True)
            for k in range(len(RED_PACK_INPUTS) - 1, len(arrays) - 1):  # wire, then every output
                back(k)
        return _red_pack_result(ins, outs)


def _red_unpack_arrays(n_streams, stream, seq, offsets, num_bytes, timestamp, ring, max_red, block_pt, optional):
    """the arrays of an unpack call as the C calls take them: (inputs stream, seq, offsets, num_bytes, timestamp, ring, block_pt - None for NULL; outputs in
    RED_UNPACK_OUTPUTS order likewise)"""
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
    n = stream.size
    seq, offsets = _u32(seq), np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32).reshape(-1)
    timestamp = _u32(timestamp) if timestamp is not None else None
    if not (seq.size == offsets.size == num_bytes.size == n) or (timestamp is not None and timestamp.size != n):
        raise ValueError("the item arrays hold one entry per item")
    ring = np.ascontiguousarray(ring, dtype=np.uint8).reshape(-1)
    if block_pt is not None:
        block_pt = _shaped(np.ascontiguousarray(block_pt, dtype=np.int32).reshape(-1), (n_streams,), "block_pt holds one entry per stream")
    m = n * (int(max_red) + 1)
    outs = [np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, np.int32) if "timestamp" in optional else None,
            np.zeros(m, np.uint8) if "gen" in optional else None, np.zeros(n, np.uint8) if "status" in optional else None,
            np.zeros(RED_UNPACK_STATS_WORDS, np.int32) if "stats" in optional else None]
    return [stream, seq, offsets, num_bytes, timestamp, ring, block_pt], outs


def plan_red_unpack(n_streams, stream, seq, offsets, num_bytes, ring, ts_step, max_red=RED_MAX_DEPTH, timestamp=None, block_pt=None, optional=RED_UNPACK_OPTIONAL,
                    ring_capacity=None):
    """The rule of DecBatch.red_unpack on the host (lc3plus_plan_red_unpack, no device needed): the parse's items stream, seq, offsets (int64), num_bytes and the
    optional timestamp [n] over ring (uint8, ring_capacity bytes of it: all by default), optional block_pt [n_streams] -> dict of stream, seq, offsets (int64),
    num_bytes, timestamp, gen (uint8) [n * (max_red + 1)] - the item arrays of ingest and probe - status (uint8) [n] and stats [RED_UNPACK_STATS_WORDS]; those of
    RED_UNPACK_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    ins, outs = _red_unpack_arrays(n_streams, stream, seq, offsets, num_bytes, timestamp, ring, max_red, block_pt, optional)
    pad = np.zeros(8, np.uint8)
    ptr = lambda a: (a if a.size else pad).ctypes.data if a is not None else None
    cap = ins[5].size if ring_capacity is None else int(ring_capacity)
    rc = load_library().lc3plus_plan_red_unpack(int(n_streams), ins[0].size, *[ptr(a) for a in ins[:6]], cap, int(max_red), ptr(ins[6]), int(ts_step),
                                                *[ptr(a) for a in outs], None, 0)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_red_unpack")
    return dict(zip(RED_UNPACK_OUTPUTS, outs))


FEC_ENCODE_INPUTS = ("n_packets", "pkt_route", "pkt_frame", "pkt_offset", "pkt_size", "pkt_status", "wire", "seq_base", "route_stats", "group", "flush", "fec_seq_base",
                     "state_in", "acc_in")
FEC_ENCODE_OPTIONAL = ("fec_flags", "fec_mask", "next_fec_seq", "route_stats")
FEC_ENCODE_OUTPUTS = ("state", "acc", "fec_wire", "n_fec", "fec_route", "fec_seq", "fec_frame", "fec_offset", "fec_size", "fec_flags", "fec_mask", "next_fec_seq",
                      "route_stats")
FEC_RECOVER_OPTIONAL = ("status", "stats")
FEC_RECOVER_OUTPUTS = ("ring", "rec_dg_offsets", "rec_dg_sizes", "rec_seq", "status", "stats")


def fec_work_bytes(n_routes, n_frames):
    """bytes of the workspace of a fec_encode call (lc3plus_fec_work_bytes); 0 for arguments the calls refuse"""
    return int(load_library().lc3plus_fec_work_bytes(int(n_routes), int(n_frames)))


def fec_recover_work_bytes(n_streams, window):
    """bytes of the workspace of a fec_recover call (lc3plus_fec_recover_work_bytes); 0 for arguments the call refuses"""
    return int(load_library().lc3plus_fec_recover_work_bytes(int(n_streams), int(window)))


def _fec_encode_arrays(pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, pkt_status, n_packets, route_stats, flush,
                       state, acc, acc_stride, max_fec_packets, optional):
    """the arrays of an encode call as the C calls take them: (inputs by name, None for a NULL one; outputs in FEC_ENCODE_OUTPUTS order; work; max_fec_packets)"""
    route = np.ascontiguousarray(pkt_route, dtype=np.int32).reshape(-1)
    m = route.size
    per = lambda a, dt, what: _shaped(np.ascontiguousarray(a, dtype=dt).reshape(-1), (m,), what)
    frame = per(pkt_frame, np.int32, "pkt_frame holds one entry per packet")
    offset = per(pkt_offset, np.int64, "pkt_offset holds one entry per packet")
    size = per(pkt_size, np.int32, "pkt_size holds one entry per packet")
    status = None if pkt_status is None else per(pkt_status, np.uint8, "pkt_status holds one entry per packet")
    seq_base = _u32(seq_base)
    R = seq_base.size
    rt = lambda a, dt, what: _shaped(np.ascontiguousarray(a, dtype=dt).reshape(-1), (R,), what)
    group = rt(group, np.int32, "group holds one entry per route")
    fec_seq_base = _shaped(_u32(fec_seq_base), (R,), "fec_seq_base holds one entry per route")
    flush = None if flush is None else rt(flush, np.uint8, "flush holds one entry per route")
    route_stats = None if route_stats is None else _shaped(np.ascontiguousarray(route_stats, dtype=np.int32), (R, EGR_STATS_WORDS), "route_stats is the egress's stats")
    if (state is None) != (acc is None):
        raise ValueError("state and acc come together")
    state_out = acc_out = None
    if state is not None:
        state = _shaped(np.ascontiguousarray(state, dtype=np.int32), (R, FEC_STATE_WORDS), "state must have shape [n_routes, FEC_STATE_WORDS]")
        acc = _shaped(np.ascontiguousarray(acc, dtype=np.uint8), (R, int(acc_stride)), "acc must have shape [n_routes, acc_stride]")
        state_out, acc_out = np.zeros_like(state), np.zeros_like(acc)
    count = np.array([m if n_packets is None else int(n_packets)], np.int64)
    wire = np.ascontiguousarray(wire, dtype=np.uint8).reshape(-1)
    fec_wire = np.array(fec_wire, dtype=np.uint8).reshape(-1)         # a copy: the call's FEC buffer starts with these contents
    q = max(R * int(n_frames), 1) if max_fec_packets is None else int(max_fec_packets)
    n = max(q, 1)
    ins = dict(n_packets=count, pkt_route=route, pkt_frame=frame, pkt_offset=offset, pkt_size=size, pkt_status=status, wire=wire, seq_base=seq_base,
               route_stats=route_stats, group=group, flush=flush, fec_seq_base=fec_seq_base, state_in=state, acc_in=acc)
    outs = [state_out, acc_out, fec_wire, np.zeros(1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64),
            np.zeros(n, np.int32), np.zeros(n, np.uint8) if "fec_flags" in optional else None, np.zeros(n, np.int32) if "fec_mask" in optional else None,
            np.zeros(R, np.int32) if "next_fec_seq" in optional else None, np.zeros((R, FEC_ROUTE_STATS_WORDS), np.int32) if "route_stats" in optional else None]
    work = np.zeros(max(fec_work_bytes(R, n_frames), 8) // 8, np.int64)
    return ins, outs, work, q


def _fec_encode_args(ins, outs, work, v, n_frames, header_room, payload_room, acc_stride, fec_stride, fec_header_room, max_fec_packets, wire_capacity, fec_capacity,
                     seq_in_place=False):
    """the C calls' arguments behind the batch; v: the pointers of FEC_ENCODE_INPUTS, then of the outputs, then of work.  seq_in_place: next_fec_seq is the array
    fec_seq_base itself"""
    k = len(FEC_ENCODE_INPUTS)
    i, o = dict(zip(FEC_ENCODE_INPUTS, v[:k])), list(v[k:k + len(outs)])
    if seq_in_place:
        o[FEC_ENCODE_OUTPUTS.index("next_fec_seq")] = i["fec_seq_base"]
    wcap = ins["wire"].size if wire_capacity is None else int(wire_capacity)
    fcap = outs[2].size if fec_capacity is None else int(fec_capacity)
    return [ins["pkt_route"].size, i["n_packets"], i["pkt_route"], i["pkt_frame"], i["pkt_offset"], i["pkt_size"], i["pkt_status"], i["wire"], wcap, int(header_room),
            int(payload_room), ins["seq_base"].size, int(n_frames), i["seq_base"], i["route_stats"], i["group"], i["flush"], i["fec_seq_base"], i["state_in"], i["acc_in"],
            o[0], o[1], int(acc_stride or 0), o[2], fcap, int(fec_stride), int(fec_header_room), int(max_fec_packets)] + list(o[3:]) + [v[-1]]


def _fec_encode_result(outs):
    r = dict(zip(FEC_ENCODE_OUTPUTS, outs))
    r["n_fec"] = int(r["n_fec"][0])
    return r


def plan_fec_encode(pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, fec_stride, header_room=12, payload_room=0,
                    fec_header_room=12, pkt_status=None, n_packets=None, route_stats=None, flush=None, state=None, acc=None, acc_stride=None, max_fec_packets=None,
                    wire_capacity=None, fec_capacity=None, optional=FEC_ENCODE_OPTIONAL, seq_in_place=False):
    """The rule of Batch.fec_encode_device / DecBatch.fec_encode_device on the host (lc3plus_plan_fec_encode, no device needed): the stamped list pkt_route,
    pkt_frame, pkt_offset (int64), pkt_size and optional pkt_status [max_packets] (n_packets of it: all by default) over wire (uint8), per route seq_base, group,
    fec_seq_base and the optional flush (uint8) and route_stats (the egress's), the previous call's state [n_routes, FEC_STATE_WORDS] with acc
    [n_routes, acc_stride], and fec_wire, the FEC buffer's contents before the call -> dict of n_fec (int), fec_route, fec_seq, fec_frame, fec_offset (int64),
    fec_size, fec_flags (uint8), fec_mask [max_fec_packets: n_routes * n_frames by default], next_fec_seq [n_routes], route_stats
    [n_routes, FEC_ROUTE_STATS_WORDS], state / acc for the next call (None without state) and fec_wire (the buffer after the call); the outputs of
    FEC_ENCODE_OPTIONAL not named in `optional` are passed as NULL and come back as None.  seq_in_place: the call gets its copy of fec_seq_base as next_fec_seq
    too, as a caller may who keeps one array.  LC3Error for arguments the C call refuses."""
    ins, outs, work, q = _fec_encode_arrays(pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, pkt_status, n_packets,
                                            route_stats, flush, state, acc, acc_stride, max_fec_packets, optional)
    pad = np.zeros(8, np.uint8)                                       # an empty array still has to be a pointer
    ptr = lambda a: (a if a.size else pad).ctypes.data if a is not None else None
    v = [ptr(ins[k]) for k in FEC_ENCODE_INPUTS] + [ptr(a) for a in outs] + [ptr(work)]
    rc = load_library().lc3plus_plan_fec_encode(*_fec_encode_args(ins, outs, work, v, n_frames, header_room, payload_room, acc_stride, fec_stride, fec_header_room, q,
                                                                  wire_capacity, fec_capacity, seq_in_place), None, 0)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_fec_encode")
    if seq_in_place:
        outs[FEC_ENCODE_OUTPUTS.index("next_fec_seq")] = ins["fec_seq_base"]
    return _fec_encode_result(outs)


class _FecEncode:
    """The send side of the generic FEC for both batch kinds (lc3plus_{enc,dec}_batch_fec_encode; include/lc3plus_batch.h "Generic FEC")."""

    def fec_encode_device(self, max_packets, d_n_packets_ptr, d_pkt_route_ptr, d_pkt_frame_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, d_wire_ptr, wire_capacity, n_routes,
                          n_frames, d_seq_base_ptr, d_group_ptr, d_fec_seq_base_ptr, d_fec_wire_ptr, fec_capacity, fec_stride, max_fec_packets, d_n_fec_ptr,
                          d_fec_route_ptr, d_fec_seq_ptr, d_fec_frame_ptr, d_fec_offset_ptr, d_fec_size_ptr, d_work_ptr, header_room=12, payload_room=0,
                          fec_header_room=12, d_pkt_status_ptr=None, d_route_stats_ptr=None, d_flush_ptr=None, d_state_in_ptr=None, d_acc_in_ptr=None,
                          d_state_out_ptr=None, d_acc_out_ptr=None, acc_stride=0, d_fec_flags_ptr=None, d_fec_mask_ptr=None, d_next_fec_seq_ptr=None,
                          d_route_stats_out_ptr=None, hip_stream=None, sync=False):
        """Raw device pointers only - the list a stamp call took with the stamp's pkt_status, the stamped wire buffer, per route seq_base, group, fec_seq_base and
        the optional flush, route_stats (the egress's) and state / accumulator pairs -> RFC 5109 parity packets behind fec_header_room bytes each at
        fec_wire + q * fec_stride, the FEC list fec_route, fec_seq, fec_frame, fec_offset (int64), fec_size [max_fec_packets] with its length n_fec (one int64) and
        the optional fec_flags (uint8), fec_mask, next_fec_seq [n_routes], route_stats_out [n_routes, FEC_ROUTE_STATS_WORDS].  work: fec_work_bytes(n_routes,
        n_frames) bytes.  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self._ssf("_fec_encode")(self.h, int(max_packets), p(d_n_packets_ptr), p(d_pkt_route_ptr), p(d_pkt_frame_ptr), p(d_pkt_offset_ptr), p(d_pkt_size_ptr),
                                      p(d_pkt_status_ptr), p(d_wire_ptr), int(wire_capacity), int(header_room), int(payload_room), int(n_routes), int(n_frames),
                                      p(d_seq_base_ptr), p(d_route_stats_ptr), p(d_group_ptr), p(d_flush_ptr), p(d_fec_seq_base_ptr), p(d_state_in_ptr), p(d_acc_in_ptr),
                                      p(d_state_out_ptr), p(d_acc_out_ptr), int(acc_stride), p(d_fec_wire_ptr), int(fec_capacity), int(fec_stride), int(fec_header_room),
                                      int(max_fec_packets), p(d_n_fec_ptr), p(d_fec_route_ptr), p(d_fec_seq_ptr), p(d_fec_frame_ptr), p(d_fec_offset_ptr),
                                      p(d_fec_size_ptr), p(d_fec_flags_ptr), p(d_fec_mask_ptr), p(d_next_fec_seq_ptr), p(d_route_stats_out_ptr), p(d_work_ptr),
                                      p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, self._ss + "_fec_encode")

    def fec_encode(self, pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, fec_stride, header_room=12, payload_room=0,
                   fec_header_room=12, pkt_status=None, n_packets=None, route_stats=None, flush=None, state=None, acc=None, acc_stride=None, max_fec_packets=None,
                   wire_capacity=None, fec_capacity=None, optional=FEC_ENCODE_OPTIONAL, poison_work=None, seq_in_place=False):
        """Host convenience: the arrays of plan_fec_encode uploaded, encoded on the device and downloaded -> the dict plan_fec_encode gives.  Device memory through
        the HIP runtime (on the current device: the batch's, unless the caller has switched), freed before it returns.  poison_work: a byte the workspace is
        filled with before the call (its contents mean nothing); seq_in_place as in plan_fec_encode."""
        ins, outs, work, q = _fec_encode_arrays(pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, pkt_status,
                                                n_packets, route_stats, flush, state, acc, acc_stride, max_fec_packets, optional)
        if poison_work is not None:
            work.view(np.uint8)[:] = int(poison_work)
        arrays = [ins[k] for k in FEC_ENCODE_INPUTS] + outs + [work]
        with _on_device(arrays) as (ptrs, back):
            rc = self._ssf("_fec_encode")(self.h, *_fec_encode_args(ins, outs, work, list(ptrs), n_frames, header_room, payload_room, acc_stride, fec_stride,
                                                                    fec_header_room, q, wire_capacity, fec_capacity, seq_in_place), None, 1)
            if rc:
                raise LC3Error(rc, self._ss + "_fec_encode")
            for k in range(len(FEC_ENCODE_INPUTS), len(arrays) - 1):
                back(k)
            if seq_in_place:
                back(FEC_ENCODE_INPUTS.index("fec_seq_base"))
                outs[FEC_ENCODE_OUTPUTS.index("next_fec_seq")] = ins["fec_seq_base"]
        return _fec_encode_result(outs)


def _fec_recover_arrays(n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, window, optional):
    """the arrays of a recover call as the C calls take them: (inputs dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc; outputs in
    FEC_RECOVER_OUTPUTS order, None for a NULL one; work)"""
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
    n = stream.size
    dg_offsets = _shaped(np.ascontiguousarray(dg_offsets, dtype=np.int64).reshape(-1), (n,), "the item arrays hold one entry per item")
    dg_sizes = _shaped(np.ascontiguousarray(dg_sizes, dtype=np.int32).reshape(-1), (n,), "the item arrays hold one entry per item")
    seq = _shaped(_u32(seq), (n,), "the item arrays hold one entry per item")
    fec_stream = np.ascontiguousarray(fec_stream, dtype=np.int32).reshape(-1)
    m = fec_stream.size
    fec_offsets = _shaped(np.ascontiguousarray(fec_offsets, dtype=np.int64).reshape(-1), (m,), "the FEC item arrays hold one entry per FEC item")
    fec_num_bytes = _shaped(np.ascontiguousarray(fec_num_bytes, dtype=np.int32).reshape(-1), (m,), "the FEC item arrays hold one entry per FEC item")
    ssrc = _shaped(_u32(ssrc), (int(n_streams),), "ssrc holds one entry per stream")
    ring = np.array(ring, dtype=np.uint8).reshape(-1)                 # a copy: the call's ring starts with these contents
    outs = [ring, np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8) if "status" in optional else None,
            np.zeros(FEC_STATS_WORDS, np.int32) if "stats" in optional else None]
    work = np.zeros(max(fec_recover_work_bytes(n_streams, window), 8) // 8, np.int64)
    return [dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc], outs, work


def _fec_recover_args(ins, outs, v, window, rec_offset, rec_stride, ring_capacity):
    """the C calls' arguments behind the batch or n_streams; v: the pointers of the inputs, the outputs and work"""
    cap = outs[0].size if ring_capacity is None else int(ring_capacity)
    return [ins[0].size, v[8], cap, v[0], v[1], v[2], v[3], ins[4].size, v[4], v[5], v[6], int(window), v[7], int(rec_offset), int(rec_stride), v[9], v[10], v[11], v[12],
            v[13], v[14]]


def plan_fec_recover(n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, rec_offset, rec_stride, window=1024,
                     ring_capacity=None, optional=FEC_RECOVER_OPTIONAL):
    """The rule of DecBatch.fec_recover on the host (lc3plus_plan_fec_recover, no device needed): the datagrams dg_offsets (int64), dg_sizes with the media parse's
    stream, seq [n_items], the FEC parse's items fec_stream, fec_offsets (int64), fec_num_bytes [n_fec] over ring (uint8, its contents before the call), ssrc
    [n_streams] -> dict of ring (after the call: recovered packets at rec_offset + f * rec_stride), rec_dg_offsets (int64), rec_dg_sizes, rec_seq, status (uint8)
    [n_fec] and stats [FEC_STATS_WORDS]; those of FEC_RECOVER_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments
    the C call refuses."""
    ins, outs, work = _fec_recover_arrays(n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, window, optional)
    pad = np.zeros(8, np.uint8)
    ptr = lambda a: (a if a.size else pad).ctypes.data if a is not None else None
    v = [ptr(a) for a in ins + outs + [work]]
    rc = load_library().lc3plus_plan_fec_recover(int(n_streams), *_fec_recover_args(ins, outs, v, window, rec_offset, rec_stride, ring_capacity), None, 0)
    if rc:
        raise LC3Error(rc, "lc3plus_plan_fec_recover")
    return dict(zip(FEC_RECOVER_OUTPUTS, outs))


RR_OPTIONAL = ("ext_seq", "item_status", "stream_stats")
RR_OUTPUTS = ("state", "blocks", "ext_seq", "item_status", "stream_stats")


def rtcp_workspace_bytes(n_items, n_streams):
    """the bytes of the workspace a DecBatch.rtcp_stats_device call over n_items items and n_streams streams needs (lc3plus_rtcp_workspace_bytes); 0 for
    arguments the call refuses"""
    return int(load_library().lc3plus_rtcp_workspace_bytes(int(n_items), int(n_streams)))


def _rtcp_arrays(stream, seq, timestamp, arrival, state, make_report, ssrc, lsr, dlsr, optional):
    """the arrays of a stats call as the C calls take them: (inputs stream, seq, timestamp, arrival, state_in, ssrc, lsr, dlsr - None for NULL; outputs in
    RR_OUTPUTS order likewise)"""
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
    n = stream.size
    seq, timestamp, arrival = _u32(seq), _u32(timestamp), _u32(arrival)
    if not (seq.size == timestamp.size == arrival.size == n):
        raise ValueError("stream, seq, timestamp and arrival hold one entry per item")
    state = _u32(state).reshape(-1, RR_STATE_WORDS) if np.asarray(state).size % RR_STATE_WORDS == 0 else None
    if state is None:
        raise ValueError("state must have shape [n_streams, RR_STATE_WORDS]")
    S = state.shape[0]
    per = [None if a is None else _u32(a) for a in (ssrc, lsr, dlsr)]
    if any(a is not None and a.size != S for a in per):
        raise ValueError("ssrc, lsr and dlsr hold one entry per stream")
    outs = [np.zeros((S, RR_STATE_WORDS), np.int32), np.zeros((S, RR_BLOCK_BYTES), np.uint8) if make_report else None,
            np.zeros(n, np.int32) if "ext_seq" in optional else None, np.zeros(n, np.uint8) if "item_status" in optional else None,
            np.zeros((S, RR_STATS_WORDS), np.int32) if "stream_stats" in optional else None]
    return [stream, seq, timestamp, arrival, np.ascontiguousarray(state)] + per, outs


def plan_rtcp_stats(stream, seq, timestamp, arrival, state, make_report=False, ssrc=None, lsr=None, dlsr=None, optional=RR_OPTIONAL):
    """The rule of DecBatch.rtcp_stats on the host (lc3plus_plan_rtcp_stats, no device needed): the parse's item arrays stream / seq / timestamp [n] and the
    arrival time of each item on its stream's RTP clock, state [n_streams, RR_STATE_WORDS] (zeros: a source that has not started), with make_report ssrc and
    optionally lsr, dlsr [n_streams] -> dict of state (the advanced state), blocks [n_streams, RR_BLOCK_BYTES] (uint8; None without make_report), ext_seq [n],
    item_status (uint8) [n] and stream_stats [n_streams, RR_STATS_WORDS]; those of RR_OPTIONAL not named in `optional` are passed as NULL and come back as
    None.  LC3Error for arguments the C call refuses."""
    ins, outs = _rtcp_arrays(stream, seq, timestamp, arrival, state, make_report, ssrc, lsr, dlsr, optional)
    pad = np.zeros(8, np.uint8)                                       # an empty array still has to be a pointer
    ptr = lambda a: (a if a.size else pad).ctypes.data if a is not None else None
    rc = load_library().lc3plus_plan_rtcp_stats(ins[0].size, *[ptr(a) for a in ins[:4]], ins[4].shape[0], ptr(ins[4]), ptr(outs[0]), 1 if make_report else 0,
                                                ptr(ins[5]), ptr(ins[6]), ptr(ins[7]), *[ptr(a) for a in outs[1:]])
    if rc:
        raise LC3Error(rc, "lc3plus_plan_rtcp_stats")
    return dict(zip(RR_OUTPUTS, outs))


SRTP_PROTECT_OUTPUTS = ("out_offset", "out_size", "out_status", "next_roc")
SRTP_UNPROTECT_OPTIONAL = ("status", "index", "stats")
SRTP_UNPROTECT_OUTPUTS = ("state", "sizes", "status", "index", "stats")


def srtp_make_context(master_key, master_salt):
    """An SRTP crypto context (lc3plus_srtp_make_context, host only): master_key (16 bytes) and master_salt (14 bytes) -> SRTP_CTX_WORDS int32 words - the
    round keys of the session cipher key, the session salt and the two SHA-1 midstates of the HMAC under the session authentication key (RFC 3711 4.3.1,
    key derivation rate 0) - as the device reads them; the caller stacks contexts into [n, SRTP_CTX_WORDS] and copies them to device memory."""
    key, salt = np.frombuffer(bytes(master_key), np.uint8), np.frombuffer(bytes(master_salt), np.uint8)
    if key.size != 16 or salt.size != 14:
        raise ValueError("master_key holds 16 bytes, master_salt 14")
    ctx = np.zeros(SRTP_CTX_WORDS, np.int32)
    rc = load_library().lc3plus_srtp_make_context(key.ctypes.data, salt.ctypes.data, ctx.ctypes.data)
    if rc:
        raise LC3Error(rc, "lc3plus_srtp_make_context")
    return ctx


def srtp_workspace_bytes(n_items, n_ssrc):
    """the bytes of the workspace a DecBatch.srtp_unprotect_device call over n_items datagrams and n_ssrc sources needs (lc3plus_srtp_workspace_bytes); 0 for
    arguments the call refuses"""
    return int(load_library().lc3plus_srtp_workspace_bytes(int(n_items), int(n_ssrc)))


# A Secure RTP suite as the calls below take it: the infix of its C symbols, the words of a context, and whether the C calls take tag_len (the AEAD suites
# have one tag length)
_SRTP_HMAC = types.SimpleNamespace(infix="_srtp", ctx_words=SRTP_CTX_WORDS, has_tag_len=True)
_SRTP_GCM = types.SimpleNamespace(infix="_srtp_gcm", ctx_words=SRTP_GCM_CTX_WORDS, has_tag_len=False)


_ptr = lambda a: (a if a.size else np.zeros(8, np.uint8)).ctypes.data if a is not None else None      # a host array for a C call; None: NULL
_dptr = lambda x: C.c_void_p(x) if x else None                                                           # a device pointer for a C call; 0 and None: NULL


def _plan_srtp_protect(suite, pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, tag_len, header_room, payload_room, next_seq,
                       n_packets, wire_capacity, dst_capacity):
    route = np.ascontiguousarray(pkt_route, dtype=np.int32).reshape(-1)
    m = route.size
    off, size = np.ascontiguousarray(pkt_offset, dtype=np.int64).reshape(-1), np.ascontiguousarray(pkt_size, dtype=np.int32).reshape(-1)
    pst = np.ascontiguousarray(pkt_status, dtype=np.uint8).reshape(-1)
    if not (off.size == size.size == pst.size == m):
        raise ValueError("the list arrays hold one entry per packet")
    ctx = np.ascontiguousarray(_u32(ctx)).reshape(-1, suite.ctx_words)
    R = ctx.shape[0]
    roc, seq_base = _u32(roc), _u32(seq_base)
    next_seq = _u32(next_seq) if next_seq is not None else None
    if roc.size != R or seq_base.size != R or (next_seq is not None and next_seq.size != R):
        raise ValueError("ctx, roc, seq_base and next_seq hold one entry per route")
    wire = np.ascontiguousarray(wire, dtype=np.uint8).reshape(-1)
    dst = np.array(dst, dtype=np.uint8).reshape(-1)                   # a copy: the call's destination starts with these contents
    count = np.array([m if n_packets is None else int(n_packets)], np.int64)
    outs = [np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(R, np.int32) if next_seq is not None else None]
    name = "lc3plus_plan%s_protect" % suite.infix
    rc = getattr(load_library(), name)(m, _ptr(count), _ptr(route), _ptr(off), _ptr(size), _ptr(pst), _ptr(wire),
                                       wire.size if wire_capacity is None else int(wire_capacity), int(header_room), int(payload_room), R, _ptr(ctx),
                                       _ptr(roc), _ptr(seq_base), _ptr(next_seq), _ptr(dst), dst.size if dst_capacity is None else int(dst_capacity),
                                       int(dst_stride), *([int(tag_len)] if suite.has_tag_len else []), *[_ptr(a) for a in outs])
    if rc:
        raise LC3Error(rc, name)
    return dict(zip(SRTP_PROTECT_OUTPUTS, outs), dst=dst)


def plan_srtp_protect(pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, tag_len=10, header_room=12, payload_room=0,
                      next_seq=None, n_packets=None, wire_capacity=None, dst_capacity=None):
    """The rule of Batch.srtp_protect_device / DecBatch.srtp_protect_device on the host (lc3plus_plan_srtp_protect, no device needed): the stamp's view of the
    egress's packet list pkt_route, pkt_offset (int64), pkt_size, pkt_status (uint8) [max_packets] (n_packets of it: all by default), the stamped wire buffer
    (uint8; wire_capacity bytes of it), per route ctx [n_routes, SRTP_CTX_WORDS], roc, seq_base and optionally next_seq [n_routes]; dst: the destination's
    contents before the call (uint8; dst_capacity bytes of it) -> dict of dst (the buffer after the call), out_offset (int64), out_size, out_status (uint8)
    [max_packets] (zero behind n_packets) and next_roc [n_routes] (None without next_seq).  LC3Error for arguments the C call refuses."""
    return _plan_srtp_protect(_SRTP_HMAC, pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, tag_len, header_room, payload_room,
                              next_seq, n_packets, wire_capacity, dst_capacity)


def _srtp_unprotect_arrays(ctx_words, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, optional, ring_capacity):
    """the arrays of an unprotect call as the C calls take them, by name (ring: a copy; None for NULL), the list's length n, n_ssrc and the ring's capacity"""
    a = types.SimpleNamespace(ring=np.array(ring, dtype=np.uint8).reshape(-1), dg_offsets=np.ascontiguousarray(dg_offsets, dtype=np.int64).reshape(-1),
                              dg_sizes=np.ascontiguousarray(dg_sizes, dtype=np.int32).reshape(-1), ssrc_key=_u32(ssrc_key),
                              ctx=np.ascontiguousarray(_u32(ctx)).reshape(-1, ctx_words), state_in=np.ascontiguousarray(_u32(state)).reshape(-1, SRTP_STATE_WORDS))
    a.n, a.n_ssrc, a.capacity = a.dg_offsets.size, a.ssrc_key.size, a.ring.size if ring_capacity is None else int(ring_capacity)
    if a.n != a.dg_sizes.size:
        raise ValueError("dg_offsets and dg_sizes hold one entry per datagram")
    if a.ctx.shape[0] != a.n_ssrc or a.state_in.shape[0] != a.n_ssrc:
        raise ValueError("ssrc_key, ctx and state hold one entry per source")
    a.state_out, a.sizes = np.zeros((a.n_ssrc, SRTP_STATE_WORDS), np.int32), np.zeros(a.n, np.int32)
    a.status, a.index = np.zeros(a.n, np.uint8) if "status" in optional else None, np.zeros(a.n, np.int64) if "index" in optional else None
    a.stats = np.zeros(SRTP_STATS_WORDS, np.int32) if "stats" in optional else None
    a.result = lambda: dict(zip(SRTP_UNPROTECT_OUTPUTS, (a.state_out, a.sizes, a.status, a.index, a.stats)), ring=a.ring)
    return a


def _plan_srtp_unprotect(suite, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity):
    a = _srtp_unprotect_arrays(suite.ctx_words, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, optional, ring_capacity)
    name = "lc3plus_plan%s_unprotect" % suite.infix
    rc = getattr(load_library(), name)(a.n, _ptr(a.ring), a.capacity, _ptr(a.dg_offsets), _ptr(a.dg_sizes), a.n_ssrc, _ptr(a.ssrc_key), _ptr(a.ctx), _ptr(a.state_in),
                                       _ptr(a.state_out), *([int(tag_len)] if suite.has_tag_len else []), _ptr(a.sizes), _ptr(a.status), _ptr(a.index), _ptr(a.stats))
    if rc:
        raise LC3Error(rc, name)
    return a.result()


def plan_srtp_unprotect(ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len=10, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
    """The rule of DecBatch.srtp_unprotect on the host (lc3plus_plan_srtp_unprotect, no device needed): ring (uint8, ring_capacity bytes of it: all by default),
    the datagrams dg_offsets (int64) / dg_sizes [n], the sources ssrc_key (ascending as uint32) with ctx [n_ssrc, SRTP_CTX_WORDS] and state [n_ssrc,
    SRTP_STATE_WORDS] (zeros: a source that has not started) -> dict of ring (the buffer after the call: accepted payloads decrypted), state (the advanced
    state), sizes [n] (rtp_parse's dg_sizes), status (uint8) [n], index (int64) [n] and stats [SRTP_STATS_WORDS]; those of SRTP_UNPROTECT_OPTIONAL not named in
    `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    return _plan_srtp_unprotect(_SRTP_HMAC, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity)


def srtp_gcm_make_context(master_key, master_salt):
    """An SRTP AES-GCM crypto context (lc3plus_srtp_gcm_make_context, host only): master_key (16 bytes: AEAD_AES_128_GCM; 32 bytes: AEAD_AES_256_GCM) and
    master_salt (12 bytes) -> SRTP_GCM_CTX_WORDS int32 words - the round keys of the session key, the number of rounds, the session salt and the GHASH table
    (RFC 7714 11, key derivation rate 0) - as the device reads them; the caller stacks contexts, of both key sizes where it likes, into
    [n, SRTP_GCM_CTX_WORDS] and copies them to device memory."""
    key, salt = np.frombuffer(bytes(master_key), np.uint8), np.frombuffer(bytes(master_salt), np.uint8)
    if key.size not in (16, 32) or salt.size != 12:
        raise ValueError("master_key holds 16 or 32 bytes, master_salt 12")
    ctx = np.zeros(SRTP_GCM_CTX_WORDS, np.int32)
    rc = load_library().lc3plus_srtp_gcm_make_context(key.ctypes.data, key.size, salt.ctypes.data, ctx.ctypes.data)
    if rc:
        raise LC3Error(rc, "lc3plus_srtp_gcm_make_context")
    return ctx


def plan_srtp_gcm_protect(pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, header_room=12, payload_room=0, next_seq=None,
                          n_packets=None, wire_capacity=None, dst_capacity=None):
    """plan_srtp_protect for the AEAD suites (lc3plus_plan_srtp_gcm_protect): the same arguments without tag_len, ctx [n_routes, SRTP_GCM_CTX_WORDS] -> the same
    dict; a protected packet is SRTP_GCM_TAG_BYTES longer than its RTP packet."""
    return _plan_srtp_protect(_SRTP_GCM, pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, None, header_room, payload_room,
                              next_seq, n_packets, wire_capacity, dst_capacity)


def plan_srtp_gcm_unprotect(ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
    """plan_srtp_unprotect for the AEAD suites (lc3plus_plan_srtp_gcm_unprotect): the same arguments without tag_len, ctx [n_ssrc, SRTP_GCM_CTX_WORDS] -> the
    same dict."""
    return _plan_srtp_unprotect(_SRTP_GCM, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, None, optional, ring_capacity)


def _srtp_protect_device(suite, self, max_packets, d_n_packets_ptr, d_pkt_route_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, d_pkt_status_ptr, d_wire_ptr, wire_capacity,
                         n_routes, d_ctx_ptr, d_roc_ptr, d_seq_base_ptr, d_dst_ptr, dst_capacity, dst_stride, d_out_offset_ptr, d_out_size_ptr, d_out_status_ptr,
                         header_room, payload_room, d_next_seq_ptr, d_next_roc_ptr, hip_stream, sync, tag_len=None):
    """the protect methods of both suites and batch kinds: called with the method's locals()"""
    p, name = _dptr, suite.infix + "_protect"
    rc = self._ssf(name)(self.h, int(max_packets), p(d_n_packets_ptr), p(d_pkt_route_ptr), p(d_pkt_offset_ptr), p(d_pkt_size_ptr), p(d_pkt_status_ptr),
                         p(d_wire_ptr), int(wire_capacity), int(header_room), int(payload_room), int(n_routes), p(d_ctx_ptr), p(d_roc_ptr), p(d_seq_base_ptr),
                         p(d_next_seq_ptr), p(d_dst_ptr), int(dst_capacity), int(dst_stride), *([int(tag_len)] if suite.has_tag_len else []), p(d_out_offset_ptr),
                         p(d_out_size_ptr), p(d_out_status_ptr), p(d_next_roc_ptr), p(hip_stream), 1 if sync else 0)
    if rc:
        raise LC3Error(rc, self._ss + name)


def _srtp_unprotect_device(suite, self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, n_ssrc, d_ssrc_key_ptr, d_ctx_ptr, d_state_in_ptr,
                           d_state_out_ptr, d_sizes_out_ptr, d_workspace_ptr, workspace_bytes, d_status_ptr, d_index_ptr, d_stats_ptr, hip_stream, sync, tag_len=None):
    """the unprotect methods of both suites: called with the method's locals()"""
    p, name = _dptr, "lc3plus_dec_batch%s_unprotect" % suite.infix
    rc = getattr(self.lib, name)(self.h, int(n_items), p(d_ring_ptr), int(ring_capacity), p(d_dg_offsets_ptr), p(d_dg_sizes_ptr), int(n_ssrc), p(d_ssrc_key_ptr),
                                 p(d_ctx_ptr), p(d_state_in_ptr), p(d_state_out_ptr), *([int(tag_len)] if suite.has_tag_len else []), p(d_sizes_out_ptr),
                                 p(d_status_ptr), p(d_index_ptr), p(d_stats_ptr), p(d_workspace_ptr), int(workspace_bytes), p(hip_stream), 1 if sync else 0)
    if rc:
        raise LC3Error(rc, name)


class _SrtpProtect:
    """The send side of Secure RTP for both batch kinds (lc3plus_{enc,dec}_batch_srtp_protect and _srtp_gcm_protect; include/lc3plus_batch.h "Secure RTP")."""

    def srtp_protect_device(self, max_packets, d_n_packets_ptr, d_pkt_route_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, d_pkt_status_ptr, d_wire_ptr, wire_capacity,
                            n_routes, d_ctx_ptr, d_roc_ptr, d_seq_base_ptr, d_dst_ptr, dst_capacity, dst_stride, d_out_offset_ptr, d_out_size_ptr,
                            d_out_status_ptr, tag_len=10, header_room=12, payload_room=0, d_next_seq_ptr=None, d_next_roc_ptr=None, hip_stream=None, sync=False):
        """Raw device pointers only - the egress's packet list as rtp_stamp_device took it with the stamp's pkt_status, the stamped wire buffer, per route ctx
        [n_routes, SRTP_CTX_WORDS], roc, seq_base and optionally next_seq -> every stamped packet as an SRTP packet (header, encrypted payload, tag of tag_len
        bytes) at dst + p * dst_stride, out_offset (int64), out_size, out_status (uint8) [max_packets] and the optional next_roc [n_routes].  Stateless: nothing
        of the batch's streams is read or written.  Queued on hip_stream; returns at once unless sync."""
        _srtp_protect_device(_SRTP_HMAC, **locals())

    def srtp_gcm_protect_device(self, max_packets, d_n_packets_ptr, d_pkt_route_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, d_pkt_status_ptr, d_wire_ptr, wire_capacity,
                                n_routes, d_ctx_ptr, d_roc_ptr, d_seq_base_ptr, d_dst_ptr, dst_capacity, dst_stride, d_out_offset_ptr, d_out_size_ptr,
                                d_out_status_ptr, header_room=12, payload_room=0, d_next_seq_ptr=None, d_next_roc_ptr=None, hip_stream=None, sync=False):
        """srtp_protect_device for the AEAD suites (lc3plus_{enc,dec}_batch_srtp_gcm_protect): the same arguments without tag_len, ctx [n_routes,
        SRTP_GCM_CTX_WORDS], routes of 16- and 32-byte keys side by side -> header, AES-GCM ciphertext and a tag of SRTP_GCM_TAG_BYTES bytes at
        dst + p * dst_stride."""
        _srtp_protect_device(_SRTP_GCM, **locals())


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


ING_OPTIONAL = ("next_base", "stats", "item_status")


def _ingest_arrays(n_streams, channels, stream, seq, offsets, num_bytes, base, info, floor, n_frames, optional):
    """the arrays of an ingest call as the C calls take them: (inputs in argument order with None for a NULL one, outputs in argument order likewise)"""
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
    n = stream.size
    def seq32(x):                                                   # sequence numbers as 32-bit words: 0 ... 2^32 - 1 and negative values both fit
        return (np.asarray(x).astype(np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    seq, base = seq32(seq), seq32(base)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32).reshape(-1)
    if not (seq.size == offsets.size == num_bytes.size == n) or base.size != n_streams:
        raise ValueError("stream, seq, offsets and num_bytes hold one entry per item, base one per stream")
    if info is not None:
        info = np.ascontiguousarray(info, dtype=np.int32)
        if info.shape != (n, channels, FRAME_INFO_WORDS):
            raise ValueError("info must have shape %s, not %s" % ((n, channels, FRAME_INFO_WORDS), info.shape))
    if floor is not None:
        floor = np.ascontiguousarray(floor, dtype=np.int32).reshape(-1)
        if floor.size != n_streams:
            raise ValueError("floor holds one entry per stream")
    cells = (max(n_streams, 0), max(int(n_frames), 0))
    outs = [np.zeros(cells, np.int64), np.zeros(cells, np.int32), np.zeros(cells, np.int32), np.zeros(cells[0], np.int32),
            np.zeros(cells[0], np.int32) if "next_base" in optional else None,
            np.zeros((cells[0], ING_STATS_WORDS), np.int32) if "stats" in optional else None,
            np.zeros(n, np.uint8) if "item_status" in optional else None]
    return [stream, seq, offsets, num_bytes, info, base, floor], outs


ING_OUTPUTS = ("offsets", "num_bytes", "cell_item", "counts", "next_base", "stats", "item_status")


def plan_ingest(n_streams, channels, stream, seq, offsets, num_bytes, base, n_frames, seq_bits=16, info=None, floor=None, optional=ING_OPTIONAL):
    """The rule of DecBatch.ingest on the host (lc3plus_plan_ingest, no device needed): the item list stream / seq / offsets / num_bytes [n], base [n_streams],
    optional probe records info [n, channels, FRAME_INFO_WORDS] and floor [n_streams] -> dict of offsets (int64), num_bytes, cell_item [n_streams, n_frames],
    counts, next_base [n_streams], stats [n_streams, ING_STATS_WORDS] and item_status [n] (uint8); those of next_base, stats and item_status not named in
    `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    ins, outs = _ingest_arrays(n_streams, channels, stream, seq, offsets, num_bytes, base, info, floor, n_frames, optional)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = load_library().lc3plus_plan_ingest(int(n_streams), int(channels), ins[0].size, *[ptr(a) for a in ins], int(seq_bits), int(n_frames),
                                            *[ptr(a) for a in outs])
    if rc:
        raise LC3Error(rc, "lc3plus_plan_ingest")
    return dict(zip(ING_OUTPUTS, outs))


class DecBatch(_StreamLifecycle, _Egress, _RtpStamp, _SrtpProtect, _RedPack, _FecEncode):
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

    def probe_device(self, d_frames_ptr, frames_capacity, d_offsets_ptr, d_num_bytes_ptr, max_frame_bytes, n_items, d_info_ptr, depth=PROBE_FULL,
                     hip_stream=None, sync=False):
        """The frame probe (lc3plus_dec_batch_probe): raw device pointers only - frames frames_capacity bytes, offsets [n_items] int64, num_bytes [n_items]
        int32, info [n_items, channels, FRAME_INFO_WORDS] int32.  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns
        at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_dec_batch_probe(self.h, p(d_frames_ptr), int(frames_capacity), p(d_offsets_ptr), p(d_num_bytes_ptr), int(max_frame_bytes),
                                              int(n_items), int(depth), p(d_info_ptr), p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_probe")

    def probe(self, payloads, depth=PROBE_FULL):
        """Host convenience: a list of stream-frames (bytes or uint8 arrays, all channels; empty = lost) packed back to back, uploaded, probed ->
        int32 [n, channels, FRAME_INFO_WORDS].  Device memory through the HIP runtime (hipMalloc / hipMemcpy on the current device: the batch's, unless the
        caller has switched), freed before it returns."""
        pl = [np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
              for x in payloads]
        nb = np.array([x.size for x in pl], np.int32)
        offs = (np.cumsum(nb, dtype=np.int64) - nb).astype(np.int64)
        buf = np.concatenate(pl + [np.zeros(4, np.uint8)])            # (never empty)
        info = np.zeros((len(pl), self.channels, FRAME_INFO_WORDS), np.int32)
        hip = C.CDLL("libamdhip64.so")
        ptrs = []
        try:
            for a in (buf, offs, nb, info):
                d = C.c_void_p()
                if hip.hipMalloc(C.byref(d), C.c_size_t(a.nbytes)) != 0:
                    raise LC3Error(1, "hipMalloc")
                ptrs.append(d)
                if hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1)) != 0:
                    raise LC3Error(1, "hipMemcpy")
            self.probe_device(ptrs[0].value, buf.size - 4, ptrs[1].value, ptrs[2].value, max(int(nb.max()), 1), len(pl), ptrs[3].value, depth, sync=True)
            if hip.hipMemcpy(C.c_void_p(info.ctypes.data), ptrs[3], C.c_size_t(info.nbytes), C.c_int(2)) != 0:
                raise LC3Error(1, "hipMemcpy")
        finally:
            for d in ptrs:
                hip.hipFree(d)
        return info

    def ingest_device(self, n_items, d_stream_ptr, d_seq_ptr, d_offsets_ptr, d_num_bytes_ptr, d_base_ptr, n_frames, d_out_offsets_ptr, d_out_num_bytes_ptr,
                      d_cell_item_ptr, d_counts_ptr, seq_bits=16, d_info_ptr=None, d_floor_ptr=None, d_next_base_ptr=None, d_stats_ptr=None,
                      d_item_status_ptr=None, hip_stream=None, sync=False):
        """Packet ingest (lc3plus_dec_batch_ingest): raw device pointers only - the item list stream, seq, num_bytes [n_items] int32 and offsets [n_items]
        int64, optional probe records info [n_items, channels, FRAME_INFO_WORDS], base and optional floor [n_streams] int32 -> out_offsets (int64),
        out_num_bytes, cell_item [n_streams, n_frames], counts [n_streams] and the optional next_base [n_streams], stats [n_streams, ING_STATS_WORDS] and
        item_status [n_items] uint8.  The tables are what decode_device_packed and set_frame_counts take.  Stateless: nothing of the batch's streams is read
        or written.  Queued on hip_stream; returns at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_dec_batch_ingest(self.h, int(n_items), p(d_stream_ptr), p(d_seq_ptr), p(d_offsets_ptr), p(d_num_bytes_ptr), p(d_info_ptr),
                                               p(d_base_ptr), p(d_floor_ptr), int(seq_bits), int(n_frames), p(d_out_offsets_ptr), p(d_out_num_bytes_ptr),
                                               p(d_cell_item_ptr), p(d_counts_ptr), p(d_next_base_ptr), p(d_stats_ptr), p(d_item_status_ptr), p(hip_stream),
                                               1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_ingest")

    def ingest(self, stream, seq, offsets, num_bytes, base, n_frames, seq_bits=16, info=None, floor=None, optional=ING_OPTIONAL):
        """Host convenience: the arrays of plan_ingest uploaded, ingested on the device and downloaded -> the dict plan_ingest gives.  Device memory through the
        HIP runtime as in probe(), freed before it returns."""
        ins, outs = _ingest_arrays(self.n_streams, self.channels, stream, seq, offsets, num_bytes, base, info, floor, n_frames, optional)
        hip = C.CDLL("libamdhip64.so")
        ptrs = []
        try:
            for a in ins + outs:
                d = C.c_void_p()                                    # stays NULL for an argument that is None
                ptrs.append(d)
                if a is None:
                    continue
                if hip.hipMalloc(C.byref(d), C.c_size_t(max(a.nbytes, 4))) != 0:
                    raise LC3Error(1, "hipMalloc")
                if hip.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1)) != 0:
                    raise LC3Error(1, "hipMemcpy")
            v = [d.value for d in ptrs]
            self.ingest_device(ins[0].size, v[0], v[1], v[2], v[3], v[5], n_frames, v[7], v[8], v[9], v[10], seq_bits, v[4], v[6], v[11], v[12], v[13], sync=True)
            for a, d in zip(outs, ptrs[7:]):
                if a is not None and hip.hipMemcpy(C.c_void_p(a.ctypes.data), d, C.c_size_t(a.nbytes), C.c_int(2)) != 0:
                    raise LC3Error(1, "hipMemcpy")
        finally:
            for d in ptrs:
                if d.value:
                    hip.hipFree(d)
        return dict(zip(ING_OUTPUTS, outs))

    def rtp_parse_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, n_ssrc, d_ssrc_key_ptr, d_ssrc_stream_ptr, d_stream_ptr,
                         d_seq_ptr, d_offsets_ptr, d_num_bytes_ptr, d_payload_type_ptr=None, payload_room=0, d_timestamp_ptr=None, d_marker_ptr=None,
                         d_status_ptr=None, d_stats_ptr=None, hip_stream=None, sync=False):
        """The receive side of the RTP framing (lc3plus_dec_batch_rtp_parse): raw device pointers only - the datagrams dg_offsets (int64) / dg_sizes [n_items] in
        ring, the senders ssrc_key (ascending as uint32) / ssrc_stream [n_ssrc], optional payload_type [n_streams] -> stream, seq, offsets (int64), num_bytes
        [n_items], as ingest_device and probe_device take them (frames = ring, seq_bits = 16), and the optional timestamp [n_items], marker, status (uint8)
        [n_items] and stats [RTP_STATS_WORDS].  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns at once unless
        sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_dec_batch_rtp_parse(self.h, int(n_items), p(d_ring_ptr), int(ring_capacity), p(d_dg_offsets_ptr), p(d_dg_sizes_ptr), int(n_ssrc),
                                                  p(d_ssrc_key_ptr), p(d_ssrc_stream_ptr), p(d_payload_type_ptr), int(payload_room), p(d_stream_ptr), p(d_seq_ptr),
                                                  p(d_offsets_ptr), p(d_num_bytes_ptr), p(d_timestamp_ptr), p(d_marker_ptr), p(d_status_ptr), p(d_stats_ptr),
                                                  p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_rtp_parse")

    def rtp_parse(self, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type=None, payload_room=0, optional=RTP_PARSE_OPTIONAL, ring_capacity=None):
        """Host convenience: the arrays of plan_rtp_parse uploaded, parsed on the device and downloaded -> the dict plan_rtp_parse gives.  Device memory through
        the HIP runtime as in probe(), freed before it returns."""
        ins, outs = _rtp_parse_arrays(self.n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type, optional)
        cap = ins[0].size if ring_capacity is None else int(ring_capacity)
        with _on_device(ins + outs) as (v, back):
            self.rtp_parse_device(ins[1].size, v[0], cap, v[1], v[2], ins[3].size, v[3], v[4], v[6], v[7], v[8], v[9], v[5], payload_room, v[10], v[11], v[12],
                                  v[13], sync=True)
            for k in range(6, 14):
                back(k)
        return dict(zip(RTP_PARSE_OUTPUTS, outs))

    def red_unpack_device(self, n_items, d_stream_ptr, d_seq_ptr, d_offsets_ptr, d_num_bytes_ptr, d_ring_ptr, ring_capacity, max_red, ts_step, d_out_stream_ptr,
                          d_out_seq_ptr, d_out_offsets_ptr, d_out_num_bytes_ptr, d_timestamp_ptr=None, d_block_pt_ptr=None, d_out_timestamp_ptr=None,
                          d_out_gen_ptr=None, d_status_ptr=None, d_stats_ptr=None, hip_stream=None, sync=False):
        """The receive side of the redundant audio (lc3plus_dec_batch_red_unpack): raw device pointers only - rtp_parse_device's stream, seq, offsets (int64),
        num_bytes and optional timestamp [n_items] as they stand, over its ring, optional block_pt [n_streams] -> out_stream, out_seq, out_offsets (int64),
        out_num_bytes [n_items * (max_red + 1)], as ingest_device and probe_device take them, and the optional out_timestamp, out_gen (uint8) of that length,
        status (uint8) [n_items] and stats [RED_UNPACK_STATS_WORDS].  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns
        at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_dec_batch_red_unpack(self.h, int(n_items), p(d_stream_ptr), p(d_seq_ptr), p(d_offsets_ptr), p(d_num_bytes_ptr), p(d_timestamp_ptr),
                                                   p(d_ring_ptr), int(ring_capacity), int(max_red), p(d_block_pt_ptr), int(ts_step), p(d_out_stream_ptr), p(d_out_seq_ptr),
                                                   p(d_out_offsets_ptr), p(d_out_num_bytes_ptr), p(d_out_timestamp_ptr), p(d_out_gen_ptr), p(d_status_ptr), p(d_stats_ptr),
                                                   p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_red_unpack")

    def red_unpack(self, stream, seq, offsets, num_bytes, ring, ts_step, max_red=RED_MAX_DEPTH, timestamp=None, block_pt=None, optional=RED_UNPACK_OPTIONAL,
                   ring_capacity=None):
        """Host convenience: the arrays of plan_red_unpack uploaded, unpacked on the device and downloaded -> the dict plan_red_unpack gives.  Device memory
        through the HIP runtime as in probe(), freed before it returns."""
        ins, outs = _red_unpack_arrays(self.n_streams, stream, seq, offsets, num_bytes, timestamp, ring, max_red, block_pt, optional)
        cap = ins[5].size if ring_capacity is None else int(ring_capacity)
        with _on_device(ins + outs) as (v, back):
            self.red_unpack_device(ins[0].size, v[0], v[1], v[2], v[3], v[5], cap, max_red, ts_step, v[7], v[8], v[9], v[10], v[4], v[6], v[11], v[12], v[13], v[14],
                                   sync=True)
            for k in range(7, 15):
                back(k)
        return dict(zip(RED_UNPACK_OUTPUTS, outs))

    def fec_recover_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, d_stream_ptr, d_seq_ptr, n_fec, d_fec_stream_ptr, d_fec_offsets_ptr,
                           d_fec_num_bytes_ptr, window, d_ssrc_ptr, rec_offset, rec_stride, d_rec_dg_offsets_ptr, d_rec_dg_sizes_ptr, d_rec_seq_ptr, d_work_ptr,
                           d_status_ptr=None, d_stats_ptr=None, hip_stream=None, sync=False):
        """The receive side of the generic FEC (lc3plus_dec_batch_fec_recover): raw device pointers only - the datagram list dg_offsets (int64), dg_sizes with the
        media parse's stream, seq [n_items], the FEC parse's fec_stream, fec_offsets (int64), fec_num_bytes [n_fec] over the ring, ssrc [n_streams] -> every media
        packet that is the only one missing of an FEC item's group rebuilt at ring + rec_offset + f * rec_stride, and rec_dg_offsets (int64), rec_dg_sizes,
        rec_seq [n_fec] - a datagram list for rtp_parse_device - with the optional status (uint8) [n_fec] and stats [FEC_STATS_WORDS].  work:
        fec_recover_work_bytes(n_streams, window) bytes.  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns at once
        unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_dec_batch_fec_recover(self.h, int(n_items), p(d_ring_ptr), int(ring_capacity), p(d_dg_offsets_ptr), p(d_dg_sizes_ptr), p(d_stream_ptr),
                                                    p(d_seq_ptr), int(n_fec), p(d_fec_stream_ptr), p(d_fec_offsets_ptr), p(d_fec_num_bytes_ptr), int(window),
                                                    p(d_ssrc_ptr), int(rec_offset), int(rec_stride), p(d_rec_dg_offsets_ptr), p(d_rec_dg_sizes_ptr), p(d_rec_seq_ptr),
                                                    p(d_status_ptr), p(d_stats_ptr), p(d_work_ptr), p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_fec_recover")

    def fec_recover(self, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, rec_offset, rec_stride, window=1024, ring_capacity=None,
                    optional=FEC_RECOVER_OPTIONAL, poison_work=None):
        """Host convenience: the arrays of plan_fec_recover uploaded, recovered on the device and downloaded -> the dict plan_fec_recover gives.  Device memory
        through the HIP runtime as in probe(), freed before it returns.  poison_work: a byte the workspace is filled with before the call."""
        ins, outs, work = _fec_recover_arrays(self.n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, window, optional)
        if poison_work is not None:
            work.view(np.uint8)[:] = int(poison_work)
        arrays = ins + outs + [work]
        with _on_device(arrays) as (v, back):
            rc = self.lib.lc3plus_dec_batch_fec_recover(self.h, *_fec_recover_args(ins, outs, list(v), window, rec_offset, rec_stride, ring_capacity), None, 1)
            if rc:
                raise LC3Error(rc, "lc3plus_dec_batch_fec_recover")
            for k in range(len(ins), len(arrays) - 1):
                back(k)
        return dict(zip(FEC_RECOVER_OUTPUTS, outs))

    def rtcp_stats_device(self, n_items, d_stream_ptr, d_seq_ptr, d_timestamp_ptr, d_arrival_ptr, n_streams, d_state_in_ptr, d_state_out_ptr, d_workspace_ptr,
                          workspace_bytes, make_report=False, d_ssrc_ptr=None, d_lsr_ptr=None, d_dlsr_ptr=None, d_blocks_ptr=None, d_ext_seq_ptr=None,
                          d_item_status_ptr=None, d_stream_stats_ptr=None, hip_stream=None, sync=False):
        """Reception reports (lc3plus_dec_batch_rtcp_stats): raw device pointers only - rtp_parse_device's stream, seq and timestamp [n_items] as they stand, the
        arrival time of each item, state_in / state_out [n_streams, RR_STATE_WORDS] (they may be one array), a workspace of rtcp_workspace_bytes(n_items,
        n_streams) bytes -> the advanced state, with make_report the report blocks [n_streams, RR_BLOCK_BYTES] (needs ssrc; lsr, dlsr optional), and the optional
        ext_seq [n_items], item_status (uint8) [n_items] and stream_stats [n_streams, RR_STATS_WORDS].  Stateless: nothing of the batch's streams is read or
        written.  Queued on hip_stream; returns at once unless sync."""
        def p(x):
            return C.c_void_p(x) if x else None
        rc = self.lib.lc3plus_dec_batch_rtcp_stats(self.h, int(n_items), p(d_stream_ptr), p(d_seq_ptr), p(d_timestamp_ptr), p(d_arrival_ptr), int(n_streams),
                                                   p(d_state_in_ptr), p(d_state_out_ptr), 1 if make_report is True else int(make_report), p(d_ssrc_ptr),
                                                   p(d_lsr_ptr), p(d_dlsr_ptr), p(d_blocks_ptr), p(d_ext_seq_ptr), p(d_item_status_ptr), p(d_stream_stats_ptr),
                                                   p(d_workspace_ptr), int(workspace_bytes), p(hip_stream), 1 if sync else 0)
        if rc:
            raise LC3Error(rc, "lc3plus_dec_batch_rtcp_stats")

    def rtcp_stats(self, stream, seq, timestamp, arrival, state, make_report=False, ssrc=None, lsr=None, dlsr=None, optional=RR_OPTIONAL):
        """Host convenience: the arrays of plan_rtcp_stats uploaded, run on the device and downloaded -> the dict plan_rtcp_stats gives.  Device memory through
        the HIP runtime as in probe(), the workspace too, freed before it returns."""
        ins, outs = _rtcp_arrays(stream, seq, timestamp, arrival, state, make_report, ssrc, lsr, dlsr, optional)
        n, S = ins[0].size, ins[4].shape[0]
        work = np.zeros(max(rtcp_workspace_bytes(n, S), 8), np.uint8)
        with _on_device(ins + outs + [work]) as (v, back):
            self.rtcp_stats_device(n, v[0], v[1], v[2], v[3], S, v[4], v[8], v[13], work.size, make_report, v[5], v[6], v[7], v[9], v[10], v[11], v[12], sync=True)
            for k in range(8, 13):
                back(k)
        return dict(zip(RR_OUTPUTS, outs))

    def _srtp_unprotect(self, suite, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity):
        a = _srtp_unprotect_arrays(suite.ctx_words, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, optional, ring_capacity)
        a.work = np.zeros(max(srtp_workspace_bytes(a.n, a.n_ssrc), 8), np.uint8)
        names = ("ring", "dg_offsets", "dg_sizes", "ssrc_key", "ctx", "state_in", "state_out", "sizes", "status", "index", "stats", "work")
        with _on_device([getattr(a, k) for k in names]) as (ptrs, back):
            d = dict(zip(names, ptrs))
            _srtp_unprotect_device(suite, self, a.n, d["ring"], a.capacity, d["dg_offsets"], d["dg_sizes"], a.n_ssrc, d["ssrc_key"], d["ctx"], d["state_in"],
                                   d["state_out"], d["sizes"], d["work"], a.work.size, d["status"], d["index"], d["stats"], None, True, tag_len)
            for k in ("ring", "state_out", "sizes", "status", "index", "stats"):
                back(names.index(k))
        return a.result()

    def srtp_unprotect_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, n_ssrc, d_ssrc_key_ptr, d_ctx_ptr, d_state_in_ptr,
                              d_state_out_ptr, d_sizes_out_ptr, d_workspace_ptr, workspace_bytes, tag_len=10, d_status_ptr=None, d_index_ptr=None, d_stats_ptr=None,
                              hip_stream=None, sync=False):
        """The receive side of Secure RTP (lc3plus_dec_batch_srtp_unprotect), in front of rtp_parse_device on the same datagram list: raw device pointers only -
        the datagrams in ring, the sources ssrc_key (ascending as uint32) with ctx [n_ssrc, SRTP_CTX_WORDS], state_in / state_out [n_ssrc, SRTP_STATE_WORDS]
        (they may be one array), a workspace of srtp_workspace_bytes(n_items, n_ssrc) bytes -> the accepted datagrams decrypted in place, sizes_out [n_items]
        (rtp_parse_device's dg_sizes), the advanced state and the optional status (uint8), index (int64) [n_items] and stats [SRTP_STATS_WORDS].  Stateless:
        nothing of the batch's streams is read or written.  Queued on hip_stream; returns at once unless sync."""
        _srtp_unprotect_device(_SRTP_HMAC, **locals())

    def srtp_unprotect(self, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len=10, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
        """Host convenience: the arrays of plan_srtp_unprotect uploaded, run on the device and downloaded -> the dict plan_srtp_unprotect gives.  Device memory
        through the HIP runtime as in probe(), the workspace too, freed before it returns."""
        return self._srtp_unprotect(_SRTP_HMAC, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity)

    def srtp_gcm_unprotect_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, n_ssrc, d_ssrc_key_ptr, d_ctx_ptr, d_state_in_ptr,
                                  d_state_out_ptr, d_sizes_out_ptr, d_workspace_ptr, workspace_bytes, d_status_ptr=None, d_index_ptr=None, d_stats_ptr=None,
                                  hip_stream=None, sync=False):
        """srtp_unprotect_device for the AEAD suites (lc3plus_dec_batch_srtp_gcm_unprotect): the same arguments without tag_len, ctx [n_ssrc,
        SRTP_GCM_CTX_WORDS], sources of 16- and 32-byte keys side by side; the workspace is srtp_workspace_bytes(n_items, n_ssrc) bytes."""
        _srtp_unprotect_device(_SRTP_GCM, **locals())

    def srtp_gcm_unprotect(self, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
        """Host convenience: the arrays of plan_srtp_gcm_unprotect uploaded, run on the device and downloaded -> the dict plan_srtp_gcm_unprotect gives."""
        return self._srtp_unprotect(_SRTP_GCM, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, None, optional, ring_capacity)

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
