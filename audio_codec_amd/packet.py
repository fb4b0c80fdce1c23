"""ctypes binding of the packet layer, the Python side of csrc/lc3_packet.c: the frame probe, packet ingest and egress, RTP, RTCP, Secure RTP (both suites), redundant
audio and generic FEC of include/lc3plus_batch.h.

A call's parameter list stands once, in PARAMS, by the header's names and in the header's order.  The argtypes (declare), the X_device methods (_device_call), the
plan_X functions (_plan) and the host conveniences X (_run) all go through it and through one caller, _invoke; tests/test_binding_header_cpu.py holds the lists
against the header.  api.py imports this module and re-exports its names; what this module needs of api.py it takes through _api()."""
import contextlib
import ctypes as C

import numpy as np


def _api():
    """api.py, which imports this module: LC3Error and load_library are its"""
    from . import api
    return api


def __getattr__(name):
    if name in ("LC3Error", "load_library", "lib_path"):               # packet.LC3Error is api.LC3Error
        return getattr(_api(), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def _lib():
    return _api().load_library()


def _check(rc, what):
    if rc:
        raise _api().LC3Error(rc, what)


# the frame orders of packed output (Batch.encode_device_packed) and of the egress's packet list
PACK_STREAM_MAJOR, PACK_FRAME_MAJOR = 0, 1
# the frame probe (DecBatch.probe, frame_info_side; include/lc3plus_batch.h "Frame probe"): depths and the record's words; its status bits and reject reasons: api.py
PROBE_SIDE, PROBE_FULL = 0, 1
FRAME_INFO_WORDS = 48
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
# ... and repair across calls (DecBatch.fec_repair, plan_fec_repair; "Generic FEC", REPAIR): the words of a stream's state, a stored media item's status, the statuses
# behind FEC_OVERFLOW
FEC_REPAIR_STATE_WORDS = 4
FEC_STORED = 0
(FEC_STALE, FEC_DUPLICATE, FEC_OVERSIZE, FEC_EXPIRED, FEC_TWIN) = range(10, 15)

# the outputs of each call as the keys of the dict its plan and its convenience return, in the header's order, and those of them a caller may leave out
ING_OPTIONAL = ("next_base", "stats", "item_status")
ING_OUTPUTS = ("offsets", "num_bytes", "cell_item", "counts", "next_base", "stats", "item_status")
EGR_OPTIONAL = ("pkt_flags", "wire_total", "next_seq", "stats", "cell_status")
EGR_OUTPUTS = ("pkt_route", "pkt_seq", "pkt_frame", "pkt_offset", "pkt_size", "pkt_flags", "n_packets", "wire_total", "next_seq", "stats", "cell_status")
RTP_PARSE_OPTIONAL = ("timestamp", "marker", "status", "stats")
RTP_PARSE_OUTPUTS = ("stream", "seq", "offsets", "num_bytes", "timestamp", "marker", "status", "stats")
RTP_STAMP_OPTIONAL = ("pkt_status", "next_ts", "next_resume")
RR_OPTIONAL = ("ext_seq", "item_status", "stream_stats")
RR_OUTPUTS = ("state", "blocks", "ext_seq", "item_status", "stream_stats")
SRTP_PROTECT_OUTPUTS = ("out_offset", "out_size", "out_status", "next_roc")
SRTP_UNPROTECT_OPTIONAL = ("status", "index", "stats")
SRTP_UNPROTECT_OUTPUTS = ("state", "sizes", "status", "index", "stats")
RED_PACK_OPTIONAL = ("red_flags", "red_blocks", "wire_total", "route_stats", "tail")
RED_PACK_OUTPUTS = ("red_offset", "red_size", "red_flags", "red_blocks", "wire_total", "route_stats")
RED_UNPACK_OPTIONAL = ("timestamp", "gen", "status", "stats")
RED_UNPACK_OUTPUTS = ("stream", "seq", "offsets", "num_bytes", "timestamp", "gen", "status", "stats")
FEC_ENCODE_OPTIONAL = ("fec_flags", "fec_mask", "next_fec_seq", "route_stats")
FEC_ENCODE_OUTPUTS = ("state", "acc", "fec_wire", "n_fec", "fec_route", "fec_seq", "fec_frame", "fec_offset", "fec_size", "fec_flags", "fec_mask", "next_fec_seq",
                      "route_stats")
FEC_RECOVER_OPTIONAL = ("status", "stats")
FEC_RECOVER_OUTPUTS = ("ring", "rec_dg_offsets", "rec_dg_sizes", "rec_seq", "status", "stats")
FEC_REPAIR_OPTIONAL = ("item_status", "fec_status", "stats")
FEC_REPAIR_STORES = ("ring", "med_seq", "med_size", "fec_store", "cell_seq", "cell_size", "cell_status", "state")
FEC_REPAIR_OUTPUTS = FEC_REPAIR_STORES + ("rec_dg_offsets", "rec_dg_sizes", "rec_seq", "item_status", "fec_status", "stats")
# the input arrays of the two calls by the plans' argument names (nothing here reads them any more)
RED_PACK_INPUTS = ("frames", "offsets", "num_bytes", "flags", "counts", "route_src", "n_packets", "pkt_route", "pkt_frame", "depth", "block_pt", "tail_bytes", "tail_sizes",
                   "wire")
FEC_ENCODE_INPUTS = ("n_packets", "pkt_route", "pkt_frame", "pkt_offset", "pkt_size", "pkt_status", "wire", "seq_base", "route_stats", "group", "flush", "fec_seq_base",
                     "state_in", "acc_in")


# ---- the parameter lists ----
_CTYPE = {"int": C.c_int, "int64": C.c_int64, "ptr": C.c_void_p}


def _params(text):
    """"int n_frames, ptr frames" -> (("n_frames", "int"), ("frames", "ptr")): a parameter list as the header has it, every pointer type a ptr"""
    return tuple((name, kind) for kind, name in (p.split() for p in text.split(",")))


# what every call of a family takes behind its front, by the header's parameter names and in its order (the X_PARAMS of lc3_packet.c)
_PROBE = _params("ptr frames, int64 frames_capacity, ptr offsets, ptr num_bytes, int max_frame_bytes, int64 n_items, int depth, ptr info")
_INGEST = _params("int64 n_items, ptr stream, ptr seq, ptr offsets, ptr num_bytes, ptr info, ptr base, ptr floor, int seq_bits, int n_frames, ptr out_offsets, "
                  "ptr out_num_bytes, ptr cell_item, ptr counts, ptr next_base, ptr stats, ptr item_status")
_EGRESS = _params("int n_frames, ptr frames, int64 frames_capacity, ptr offsets, ptr num_bytes, int max_frame_bytes, ptr flags, int skip_mask, ptr counts, int n_routes, "
                  "ptr route_src, ptr seq_base, int seq_bits, int order, ptr wire, int64 wire_capacity, int header_room, int align, ptr pkt_route, ptr pkt_seq, "
                  "ptr pkt_frame, ptr pkt_offset, ptr pkt_size, ptr pkt_flags, ptr n_packets, ptr wire_total, ptr next_seq, ptr stats, ptr cell_status, ptr work")
_RTP_PARSE = _params("int64 n_items, ptr ring, int64 ring_capacity, ptr dg_offsets, ptr dg_sizes, int n_ssrc, ptr ssrc_key, ptr ssrc_stream, ptr payload_type, "
                     "int payload_room, ptr stream, ptr seq, ptr offsets, ptr num_bytes, ptr timestamp, ptr marker, ptr status, ptr stats")
_RTP_STAMP = _params("int64 max_packets, ptr n_packets, ptr pkt_route, ptr pkt_seq, ptr pkt_frame, ptr pkt_offset, ptr pkt_size, ptr pkt_flags, int n_routes, int n_frames, "
                     "ptr ssrc, ptr ts_base, ptr payload_type, int ts_step, int marker_mode, ptr cell_status, ptr resume, ptr route_stats, ptr wire, int64 wire_capacity, "
                     "int header_room, int payload_room, ptr pkt_status, ptr next_ts, ptr next_resume")
_RTCP_STATS = _params("int64 n_items, ptr stream, ptr seq, ptr timestamp, ptr arrival, int n_streams, ptr state_in, ptr state_out, int make_report, ptr ssrc, ptr lsr, "
                      "ptr dlsr, ptr blocks, ptr ext_seq, ptr item_status, ptr stream_stats")
_SRTP_PROTECT = _params("int64 max_packets, ptr n_packets, ptr pkt_route, ptr pkt_offset, ptr pkt_size, ptr pkt_status, ptr wire, int64 wire_capacity, int header_room, "
                        "int payload_room, int n_routes, ptr ctx, ptr roc, ptr seq_base, ptr next_seq, ptr dst, int64 dst_capacity, int64 dst_stride, int tag_len, "
                        "ptr out_offset, ptr out_size, ptr out_status, ptr next_roc")
_SRTP_UNPROTECT = _params("int64 n_items, ptr ring, int64 ring_capacity, ptr dg_offsets, ptr dg_sizes, int n_ssrc, ptr ssrc_key, ptr ctx, ptr state_in, ptr state_out, "
                          "int tag_len, ptr sizes_out, ptr status, ptr index, ptr stats")
_RED_PACK = _params("int n_frames, ptr frames, int64 frames_capacity, ptr offsets, ptr num_bytes, int max_frame_bytes, ptr flags, int skip_mask, ptr counts, int n_routes, "
                    "ptr route_src, int64 max_packets, ptr n_packets, ptr pkt_route, ptr pkt_frame, int max_depth, ptr depth, ptr block_pt, int ts_step, "
                    "int max_packet_bytes, ptr tail_bytes_in, ptr tail_sizes_in, int tail_stride, ptr tail_bytes_out, ptr tail_sizes_out, ptr wire, int64 wire_capacity, "
                    "int header_room, int align, ptr red_offset, ptr red_size, ptr red_flags, ptr red_blocks, ptr wire_total, ptr route_stats, ptr work")
_RED_UNPACK = _params("int64 n_items, ptr stream, ptr seq, ptr offsets, ptr num_bytes, ptr timestamp, ptr ring, int64 ring_capacity, int max_red, ptr block_pt, int ts_step, "
                      "ptr out_stream, ptr out_seq, ptr out_offsets, ptr out_num_bytes, ptr out_timestamp, ptr out_gen, ptr status, ptr stats")
_FEC_ENCODE = _params("int64 max_packets, ptr n_packets, ptr pkt_route, ptr pkt_frame, ptr pkt_offset, ptr pkt_size, ptr pkt_status, ptr wire, int64 wire_capacity, "
                      "int header_room, int payload_room, int n_routes, int n_frames, ptr seq_base, ptr route_stats, ptr group, ptr flush, ptr fec_seq_base, ptr state_in, "
                      "ptr acc_in, ptr state_out, ptr acc_out, int acc_stride, ptr fec_wire, int64 fec_capacity, int64 fec_stride, int fec_header_room, "
                      "int64 max_fec_packets, ptr n_fec, ptr fec_route, ptr fec_seq, ptr fec_frame, ptr fec_offset, ptr fec_size, ptr fec_flags, ptr fec_mask, "
                      "ptr next_fec_seq, ptr route_stats_out, ptr work")
_FEC_RECOVER = _params("int64 n_items, ptr ring, int64 ring_capacity, ptr dg_offsets, ptr dg_sizes, ptr stream, ptr seq, int64 n_fec, ptr fec_stream, ptr fec_offsets, "
                       "ptr fec_num_bytes, int window, ptr ssrc, int64 rec_offset, int64 rec_stride, ptr rec_dg_offsets, ptr rec_dg_sizes, ptr rec_seq, ptr status, "
                       "ptr stats, ptr work")
_FEC_REPAIR = _params("int64 n_items, ptr ring, int64 ring_capacity, ptr dg_offsets, ptr dg_sizes, ptr stream, ptr seq, int64 n_fec, ptr fec_stream, ptr fec_offsets, "
                      "ptr fec_num_bytes, ptr fec_seq, ptr ssrc, int64 med_offset, int med_slots, int med_stride, ptr med_seq, ptr med_size, ptr fec_store, int fec_slots, "
                      "int fec_stride, ptr cell_seq, ptr cell_size, ptr cell_status, ptr state, int passes, ptr rec_dg_offsets, ptr rec_dg_sizes, ptr rec_seq, "
                      "ptr item_status, ptr fec_status, ptr stats, ptr work")
# ... what stands in front of it and behind it
_BATCH, _STREAMS, _NOTHING = _params("ptr batch"), _params("int n_streams"), ()
_QUEUED = _params("ptr hip_stream, int sync")
_WORKSPACE = _params("ptr workspace, int64 workspace_bytes") + _QUEUED

PARAMS = {}                                                             # C symbol -> its whole parameter list


def _family(name, params, plan_front, plan_tail, batch_tail=_QUEUED, kinds=("enc", "dec")):
    """the symbols of a call family: lc3plus_plan_NAME and lc3plus_{enc,dec}_batch_NAME (the receive side: dec alone)"""
    PARAMS["lc3plus_plan_" + name] = plan_front + params + plan_tail
    for kind in kinds:
        PARAMS["lc3plus_%s_batch_%s" % (kind, name)] = _BATCH + params + batch_tail


PARAMS["lc3plus_dec_batch_probe"] = _BATCH + _PROBE + _QUEUED           # no plan of it here: the SIDE depth on the host is api.py's frame_info_side
_family("ingest", _INGEST, _params("int n_streams, int channels"), _NOTHING, kinds=("dec",))
_family("egress", _EGRESS, _STREAMS, _QUEUED)
_family("rtp_parse", _RTP_PARSE, _STREAMS, _QUEUED, kinds=("dec",))
_family("rtp_stamp", _RTP_STAMP, _NOTHING, _QUEUED)
_family("rtcp_stats", _RTCP_STATS, _NOTHING, _NOTHING, batch_tail=_WORKSPACE, kinds=("dec",))
for _suite, _drop in (("srtp", ()), ("srtp_gcm", ("tag_len",))):       # the AEAD suites have one tag length: the same lists without tag_len
    _family(_suite + "_protect", tuple(p for p in _SRTP_PROTECT if p[0] not in _drop), _NOTHING, _NOTHING)
    _family(_suite + "_unprotect", tuple(p for p in _SRTP_UNPROTECT if p[0] not in _drop), _NOTHING, _NOTHING, batch_tail=_WORKSPACE, kinds=("dec",))
_family("red_pack", _RED_PACK, _STREAMS, _QUEUED)
_family("red_unpack", _RED_UNPACK, _STREAMS, _QUEUED, kinds=("dec",))
_family("fec_encode", _FEC_ENCODE, _NOTHING, _QUEUED)
_family("fec_recover", _FEC_RECOVER, _STREAMS, _QUEUED, kinds=("dec",))
_family("fec_repair", _FEC_REPAIR, _STREAMS, _QUEUED, kinds=("dec",))
# the host-only helpers; those named *_bytes return an int64_t
PARAMS.update({"lc3plus_" + name: _params(text) for name, text in (
    ("egress_work_bytes", "int n_routes, int n_frames"), ("red_work_bytes", "int64 max_packets"), ("fec_work_bytes", "int n_routes, int n_frames"),
    ("fec_recover_work_bytes", "int n_streams, int window"), ("fec_repair_work_bytes", "int n_streams, int med_slots, int fec_slots"), ("rtcp_workspace_bytes", "int64 n_items, int n_streams"),
    ("srtp_workspace_bytes", "int64 n_items, int n_ssrc"), ("rtp_sort_ssrc", "int n, ptr ssrc_key, ptr ssrc_stream"),
    ("srtp_make_context", "ptr master_key, ptr master_salt, ptr ctx"), ("srtp_gcm_make_context", "ptr master_key, int key_bytes, ptr master_salt, ptr ctx"))})


def declare(L):
    """argtypes and restypes of every symbol of lc3_packet.c, from PARAMS (also for the stub build of the host code)"""
    for symbol, params in PARAMS.items():
        getattr(L, symbol).argtypes = [_CTYPE[kind] for _, kind in params]
        if symbol.endswith("_bytes"):
            getattr(L, symbol).restype = C.c_int64


# ---- the one caller and what runs through it ----
_PAD = np.zeros(8, np.uint8)


def _host(a):
    """a host array as a pointer for a C call; None: NULL; an empty array still has to be a pointer"""
    return (a if a.size else _PAD).ctypes.data if a is not None else None


def _dev(x):
    """a device pointer for a C call; 0 and None: NULL"""
    return C.c_void_p(x) if x else None


def _invoke(lib, symbol, values, pointer):
    """The C function `symbol` called with the values of its parameters by header name, in PARAMS' order: int() of an integer, pointer() - _host or _dev - of a
    pointer, 1 or 0 for sync.  LC3Error with the symbol's name for what it refuses."""
    convert = {"int": int, "int64": int, "ptr": pointer}
    values = dict(values, sync=1 if values.get("sync") else 0)
    _check(getattr(lib, symbol)(*[convert[kind](values[name]) for name, kind in PARAMS[symbol]]), symbol)


def _device_call(symbol, args):
    """The body of an X_device method, given its locals(): header parameter NAME is the method's argument d_NAME_ptr, or its argument NAME where it has no such;
    batch is the handle."""
    self = args["self"]
    values = {name: args.get("d_%s_ptr" % name, args.get(name)) for name, _ in PARAMS[symbol]}
    _invoke(self.lib, symbol, dict(values, batch=self.h.value), _dev)


@contextlib.contextmanager
def _on_device(values, back):
    """A call's values by name with every array (None: a NULL pointer) in device memory through the HIP runtime (hipMalloc / hipMemcpy on the current device) -> the
    values with the device pointer in place of the array.  An array that stands under two names is one buffer, as it is one pointer to a plan.  When the block ends
    without an error the buffers of the names in `back` are copied into their arrays; everything is freed at the end."""
    hip = C.CDLL("libamdhip64.so")
    bufs = {}                                                           # id(array) -> its device buffer

    def copy(dst, src, nbytes, kind):
        if nbytes and hip.hipMemcpy(dst, src, C.c_size_t(nbytes), C.c_int(kind)) != 0:
            raise _api().LC3Error(1, "hipMemcpy")
    try:
        for a in values.values():
            if isinstance(a, np.ndarray) and id(a) not in bufs:
                bufs[id(a)] = d = C.c_void_p()
                if hip.hipMalloc(C.byref(d), C.c_size_t(max(a.nbytes, 8))) != 0:
                    raise _api().LC3Error(1, "hipMalloc")
                copy(d, C.c_void_p(a.ctypes.data), a.nbytes, 1)
        yield {k: bufs[id(a)].value if isinstance(a, np.ndarray) else a for k, a in values.items()}
        for a in (values[k] for k in back):
            if a is not None:
                copy(C.c_void_p(a.ctypes.data), bufs[id(a)], a.nbytes, 2)
    finally:
        for d in bufs.values():
            if d.value:
                hip.hipFree(d)


def _names(v, keys):
    """the header's names of what a result holds under `keys`: key K is the parameter out_K or K_out where the call has such a one, K itself otherwise"""
    return tuple("out_" + k if "out_" + k in v else k + "_out" if k + "_out" in v else k for k in keys)


def _result(v, keys, ints=()):
    """the dict a plan or a convenience returns, out of the call's values; those of `ints` as the one number they hold (None stays None)"""
    r = {k: v[name] for k, name in zip(keys, _names(v, keys))}
    r.update({k: int(r[k][0]) for k in ints if r[k] is not None})
    return r


def _plan(symbol, v, keys, ints=(), **front):
    """plan_X: the call's values (_X_arrays) as they stand in host memory, nothing queued -> the result"""
    _invoke(_lib(), symbol, dict(v, hip_stream=None, sync=0, **front), _host)
    return _result(v, keys, ints)


def _run(batch, symbol, v, keys, ints=()):
    """The host convenience X: the call's values (_X_arrays) uploaded, the batch's call made and waited for, what the result holds downloaded -> the result.  Device
    memory through the HIP runtime (_on_device), freed before it returns."""
    with _on_device(v, _names(v, keys)) as d:
        _invoke(batch.lib, symbol, dict(d, batch=batch.h.value, hip_stream=None, sync=1), _dev)
    return _result(v, keys, ints)


def _u32(x):
    """32-bit words however they are given: 0 ... 2^32 - 1 and negative values both fit"""
    return (np.asarray(x).astype(np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _shaped(a, shape, what):
    if a.shape != tuple(shape):
        raise ValueError(what)
    return a


# ---- packet egress ----
def egress_work_bytes(n_routes, n_frames):
    """bytes of the workspace of an egress call (lc3plus_egress_work_bytes); 0 for a shape the calls refuse"""
    return int(_lib().lc3plus_egress_work_bytes(int(n_routes), int(n_frames)))


def _egress_arrays(n_streams, frames, offsets, num_bytes, seq_base, max_frame_bytes, flags, skip_mask, counts, route_src, seq_bits, order, wire, wire_capacity,
                   header_room, align, optional, frames_capacity):
    """the values of an egress call by header parameter name: the arrays as the C calls take them (None for a NULL one), the outputs and the workspace among them"""
    frames = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    num_bytes = np.ascontiguousarray(num_bytes, dtype=np.int32)
    if offsets.ndim != 2 or offsets.shape != num_bytes.shape or offsets.shape[0] != n_streams:
        raise ValueError("offsets and num_bytes must have shape [n_streams, n_frames]")
    T = offsets.shape[1]
    seq_base = _u32(seq_base)
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
    return dict(n_frames=T, frames=frames, frames_capacity=frames.size if frames_capacity is None else frames_capacity, offsets=offsets, num_bytes=num_bytes,
                max_frame_bytes=max_frame_bytes, flags=flags, skip_mask=skip_mask, counts=counts, n_routes=R, route_src=route_src, seq_base=seq_base, seq_bits=seq_bits,
                order=order, wire=wire, wire_capacity=(wire.size if wire is not None else 0) if wire_capacity is None else wire_capacity, header_room=header_room,
                align=align, pkt_route=np.zeros(n, np.int32), pkt_seq=np.zeros(n, np.int32), pkt_frame=np.zeros(n, np.int32), pkt_offset=np.zeros(n, np.int64),
                pkt_size=np.zeros(n, np.int32), pkt_flags=np.zeros(n, np.uint8) if "pkt_flags" in optional else None, n_packets=np.zeros(1, np.int64),
                wire_total=np.zeros(1, np.int64) if "wire_total" in optional else None, next_seq=np.zeros(R, np.int32) if "next_seq" in optional else None,
                stats=np.zeros((R, EGR_STATS_WORDS), np.int32) if "stats" in optional else None,
                cell_status=np.zeros((R, T), np.uint8) if "cell_status" in optional else None, work=np.zeros(max(egress_work_bytes(R, T), 8) // 8, np.int64))


def plan_egress(n_streams, frames, offsets, num_bytes, seq_base, max_frame_bytes, flags=None, skip_mask=0, counts=None, route_src=None, seq_bits=16,
                order=PACK_STREAM_MAJOR, wire=None, wire_capacity=None, header_room=0, align=1, optional=EGR_OPTIONAL, frames_capacity=None):
    """The rule of Batch.egress / DecBatch.egress on the host (lc3plus_plan_egress, no device needed): frames (uint8, frames_capacity bytes of it: all by
    default), offsets (int64) / num_bytes [n_streams, n_frames], seq_base [n_routes]; optional flags [n_streams, n_frames] with skip_mask, counts [n_streams],
    route_src [n_routes]; wire: None (in place) or the wire buffer's contents before the call (uint8; wire_capacity bytes of it: all by default).
    -> dict of the list arrays pkt_route, pkt_seq, pkt_frame, pkt_offset (int64), pkt_size, pkt_flags (uint8) [n_routes * n_frames] (zero behind n_packets),
    n_packets, wire_total (ints), next_seq [n_routes], stats [n_routes, EGR_STATS_WORDS], cell_status [n_routes, n_frames] (uint8) and wire (the buffer after
    the call, or None); the outputs of EGR_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call
    refuses."""
    v = _egress_arrays(n_streams, frames, offsets, num_bytes, seq_base, max_frame_bytes, flags, skip_mask, counts, route_src, seq_bits, order, wire, wire_capacity,
                       header_room, align, optional, frames_capacity)
    return _plan("lc3plus_plan_egress", v, EGR_OUTPUTS + ("wire",), ("n_packets", "wire_total"), n_streams=n_streams)


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
        _device_call(self._ss + "_egress", locals())

    def egress(self, frames, offsets, num_bytes, seq_base, max_frame_bytes, flags=None, skip_mask=0, counts=None, route_src=None, seq_bits=16,
               order=PACK_STREAM_MAJOR, wire=None, wire_capacity=None, header_room=0, align=1, optional=EGR_OPTIONAL, frames_capacity=None):
        """Host convenience: the arrays of plan_egress uploaded, the egress run on the device and downloaded -> the dict plan_egress gives.  Device memory through
        the HIP runtime (hipMalloc / hipMemcpy on the current device: the batch's, unless the caller has switched), freed before it returns."""
        v = _egress_arrays(self.n_streams, frames, offsets, num_bytes, seq_base, max_frame_bytes, flags, skip_mask, counts, route_src, seq_bits, order, wire,
                           wire_capacity, header_room, align, optional, frames_capacity)
        return _run(self, self._ss + "_egress", v, EGR_OUTPUTS + ("wire",), ("n_packets", "wire_total"))


# ---- RTP framing ----
def rtp_sort_ssrc(ssrc_key, ssrc_stream):
    """An SSRC table in the order rtp_parse needs (lc3plus_rtp_sort_ssrc): -> (keys ascending as uint32, as int32 words; each key's stream).  LC3Error for an
    empty table and for a key that occurs twice."""
    key, stream = _u32(ssrc_key).copy(), np.array(ssrc_stream, dtype=np.int32).reshape(-1)
    if key.size != stream.size:
        raise ValueError("ssrc_key and ssrc_stream hold one entry per sender")
    _check(_lib().lc3plus_rtp_sort_ssrc(key.size, key.ctypes.data if key.size else None, stream.ctypes.data if stream.size else None), "lc3plus_rtp_sort_ssrc")
    return key, stream


def _rtp_parse_arrays(n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type, payload_room, optional, ring_capacity):
    """the values of a parse call by header parameter name: the arrays as the C calls take them (None for a NULL one), the outputs among them"""
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
    return dict(n_items=n, ring=ring, ring_capacity=ring.size if ring_capacity is None else ring_capacity, dg_offsets=dg_offsets, dg_sizes=dg_sizes, n_ssrc=key.size,
                ssrc_key=key, ssrc_stream=stream, payload_type=payload_type, payload_room=payload_room, stream=np.zeros(n, np.int32), seq=np.zeros(n, np.int32),
                offsets=np.zeros(n, np.int64), num_bytes=np.zeros(n, np.int32), timestamp=np.zeros(n, np.int32) if "timestamp" in optional else None,
                marker=np.zeros(n, np.uint8) if "marker" in optional else None, status=np.zeros(n, np.uint8) if "status" in optional else None,
                stats=np.zeros(RTP_STATS_WORDS, np.int32) if "stats" in optional else None)


def plan_rtp_parse(n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type=None, payload_room=0, optional=RTP_PARSE_OPTIONAL,
                   ring_capacity=None):
    """The rule of DecBatch.rtp_parse on the host (lc3plus_plan_rtp_parse, no device needed): ring (uint8, ring_capacity bytes of it: all by default), the
    datagrams dg_offsets (int64) / dg_sizes [n], the senders ssrc_key (ascending as uint32: rtp_sort_ssrc) / ssrc_stream, optional payload_type [n_streams]
    -> dict of stream, seq, offsets (int64), num_bytes [n] - the item arrays of ingest and probe - and timestamp [n], marker, status (uint8) [n] and stats
    [RTP_STATS_WORDS]; those of RTP_PARSE_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call
    refuses."""
    v = _rtp_parse_arrays(n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type, payload_room, optional, ring_capacity)
    return _plan("lc3plus_plan_rtp_parse", v, RTP_PARSE_OUTPUTS, n_streams=n_streams)


def _rtp_stamp_arrays(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type, ts_step, n_frames, wire, header_room, payload_room, pkt_flags,
                      n_packets, marker_mode, cell_status, resume, route_stats, wire_capacity, optional):
    """the values of a stamp call by header parameter name: the arrays as the C calls take them (None for a NULL one; wire a copy), the outputs among them"""
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
    return dict(max_packets=m, n_packets=count, pkt_route=route, pkt_seq=seq, pkt_frame=frame, pkt_offset=off, pkt_size=size, pkt_flags=flags, n_routes=R,
                n_frames=n_frames, ssrc=ssrc, ts_base=ts_base, payload_type=payload_type, ts_step=ts_step, marker_mode=marker_mode, cell_status=cell_status,
                resume=resume, route_stats=route_stats, wire=wire, wire_capacity=wire.size if wire_capacity is None else wire_capacity, header_room=header_room,
                payload_room=payload_room, pkt_status=np.zeros(m, np.uint8) if "pkt_status" in optional else None,
                next_ts=np.zeros(R, np.int32) if "next_ts" in optional else None, next_resume=np.zeros(R, np.uint8) if "next_resume" in optional else None)


def plan_rtp_stamp(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type, ts_step, n_frames, wire, header_room=12, payload_room=0,
                   pkt_flags=None, n_packets=None, marker_mode=RTP_MARKER_NEVER, cell_status=None, resume=None, route_stats=None, wire_capacity=None,
                   optional=RTP_STAMP_OPTIONAL):
    """The rule of Batch.rtp_stamp / DecBatch.rtp_stamp on the host (lc3plus_plan_rtp_stamp, no device needed): the egress's packet list pkt_* [max_packets]
    (n_packets of it: all by default), per route ssrc, ts_base, payload_type [n_routes], optional cell_status [n_routes, n_frames], resume [n_routes] and
    route_stats [n_routes, EGR_STATS_WORDS] (the egress's stats); wire: the wire buffer's contents before the call (uint8; wire_capacity bytes of it: all by
    default) -> dict of wire (the buffer after the call), pkt_status (uint8) [max_packets] (zero behind n_packets), next_ts [n_routes] and next_resume (uint8)
    [n_routes]; those of RTP_STAMP_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    v = _rtp_stamp_arrays(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type, ts_step, n_frames, wire, header_room, payload_room,
                          pkt_flags, n_packets, marker_mode, cell_status, resume, route_stats, wire_capacity, optional)
    return _plan("lc3plus_plan_rtp_stamp", v, RTP_STAMP_OPTIONAL + ("wire",))


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
        _device_call(self._ss + "_rtp_stamp", locals())

    def rtp_stamp(self, pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type, ts_step, n_frames, wire, header_room=12, payload_room=0,
                  pkt_flags=None, n_packets=None, marker_mode=RTP_MARKER_NEVER, cell_status=None, resume=None, route_stats=None, wire_capacity=None,
                  optional=RTP_STAMP_OPTIONAL):
        """Host convenience: the arrays of plan_rtp_stamp uploaded, stamped on the device and downloaded -> the dict plan_rtp_stamp gives.  Device memory through
        the HIP runtime (on the current device: the batch's, unless the caller has switched), freed before it returns."""
        v = _rtp_stamp_arrays(pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type, ts_step, n_frames, wire, header_room, payload_room,
                              pkt_flags, n_packets, marker_mode, cell_status, resume, route_stats, wire_capacity, optional)
        return _run(self, self._ss + "_rtp_stamp", v, RTP_STAMP_OPTIONAL + ("wire",))


# ---- redundant audio ----
def red_work_bytes(max_packets):
    """bytes of the workspace of a red_pack call (lc3plus_red_work_bytes); 0 for a max_packets the calls refuse"""
    return int(_lib().lc3plus_red_work_bytes(int(max_packets)))


def red_tail_stride(max_frame_bytes):
    """the smallest tail_stride a red_pack call takes for frames of up to max_frame_bytes bytes"""
    return (min(int(max_frame_bytes), 1023) + 15) & ~15


def _red_pack_arrays(n_streams, frames, offsets, num_bytes, max_frame_bytes, pkt_route, pkt_frame, block_pt, ts_step, wire, max_depth, depth, max_packet_bytes, n_packets,
                     flags, skip_mask, counts, route_src, tail_bytes, tail_sizes, tail_stride, wire_capacity, header_room, align, optional, frames_capacity):
    """the values of a pack call by header parameter name: the arrays as the C calls take them (None for a NULL one; wire a copy), the outputs and the workspace
    among them"""
    stride = red_tail_stride(max_frame_bytes) if tail_stride is None else int(tail_stride)
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
    tail_bytes = opt(tail_bytes, np.uint8, (n_streams, D, stride), "tail_bytes must have shape [n_streams, max_depth, tail_stride]")
    tail_sizes = opt(tail_sizes, np.int32, (n_streams, D), "tail_sizes must have shape [n_streams, max_depth]")
    count = np.array([m if n_packets is None else int(n_packets)], np.int64)
    wire = np.array(wire, dtype=np.uint8).reshape(-1)                 # a copy: the call's wire buffer starts with these contents
    tail = "tail" in optional
    return dict(n_frames=offsets.shape[1], frames=frames, frames_capacity=frames.size if frames_capacity is None else frames_capacity, offsets=offsets,
                num_bytes=num_bytes, max_frame_bytes=max_frame_bytes, flags=flags, skip_mask=skip_mask, counts=counts, n_routes=R, route_src=route_src, max_packets=m,
                n_packets=count, pkt_route=route, pkt_frame=frame, max_depth=max_depth, depth=depth, block_pt=block_pt, ts_step=ts_step,
                max_packet_bytes=max_packet_bytes, tail_bytes_in=tail_bytes, tail_sizes_in=tail_sizes, tail_stride=stride,
                tail_bytes_out=np.zeros((n_streams, D, stride), np.uint8) if tail else None, tail_sizes_out=np.zeros((n_streams, D), np.int32) if tail else None,
                wire=wire, wire_capacity=wire.size if wire_capacity is None else wire_capacity, header_room=header_room, align=align,
                red_offset=np.zeros(m, np.int64), red_size=np.zeros(m, np.int32), red_flags=np.zeros(m, np.uint8) if "red_flags" in optional else None,
                red_blocks=np.zeros(m, np.uint8) if "red_blocks" in optional else None, wire_total=np.zeros(1, np.int64) if "wire_total" in optional else None,
                route_stats=np.zeros((R, RED_STATS_WORDS), np.int32) if "route_stats" in optional else None,
                work=np.zeros(max(red_work_bytes(max(m, 1)), 8) // 8, np.int64))


_RED_PACK_RESULT = RED_PACK_OUTPUTS + ("tail_bytes", "tail_sizes", "wire")


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
    v = _red_pack_arrays(n_streams, frames, offsets, num_bytes, max_frame_bytes, pkt_route, pkt_frame, block_pt, ts_step, wire, max_depth, depth, max_packet_bytes,
                         n_packets, flags, skip_mask, counts, route_src, tail_bytes, tail_sizes, tail_stride, wire_capacity, header_room, align, optional, frames_capacity)
    return _plan("lc3plus_plan_red_pack", v, _RED_PACK_RESULT, ("wire_total",), n_streams=n_streams)


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
        _device_call(self._ss + "_red_pack", locals())

    def red_pack(self, frames, offsets, num_bytes, max_frame_bytes, pkt_route, pkt_frame, block_pt, ts_step, wire, max_depth=1, depth=None, max_packet_bytes=1 << 30,
                 n_packets=None, flags=None, skip_mask=0, counts=None, route_src=None, tail_bytes=None, tail_sizes=None, tail_stride=None, wire_capacity=None,
                 header_room=12, align=1, optional=RED_PACK_OPTIONAL, frames_capacity=None):
        """Host convenience: the arrays of plan_red_pack uploaded, packed on the device and downloaded -> the dict plan_red_pack gives.  Device memory through the
        HIP runtime (on the current device: the batch's, unless the caller has switched), freed before it returns."""
        v = _red_pack_arrays(self.n_streams, frames, offsets, num_bytes, max_frame_bytes, pkt_route, pkt_frame, block_pt, ts_step, wire, max_depth, depth,
                             max_packet_bytes, n_packets, flags, skip_mask, counts, route_src, tail_bytes, tail_sizes, tail_stride, wire_capacity, header_room, align,
                             optional, frames_capacity)
        return _run(self, self._ss + "_red_pack", v, _RED_PACK_RESULT, ("wire_total",))


def _red_unpack_arrays(n_streams, stream, seq, offsets, num_bytes, ring, ts_step, max_red, timestamp, block_pt, optional, ring_capacity):
    """the values of an unpack call by header parameter name: the arrays as the C calls take them (None for a NULL one), the outputs among them"""
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
    return dict(n_items=n, stream=stream, seq=seq, offsets=offsets, num_bytes=num_bytes, timestamp=timestamp, ring=ring,
                ring_capacity=ring.size if ring_capacity is None else ring_capacity, max_red=max_red, block_pt=block_pt, ts_step=ts_step,
                out_stream=np.zeros(m, np.int32), out_seq=np.zeros(m, np.int32), out_offsets=np.zeros(m, np.int64), out_num_bytes=np.zeros(m, np.int32),
                out_timestamp=np.zeros(m, np.int32) if "timestamp" in optional else None, out_gen=np.zeros(m, np.uint8) if "gen" in optional else None,
                status=np.zeros(n, np.uint8) if "status" in optional else None, stats=np.zeros(RED_UNPACK_STATS_WORDS, np.int32) if "stats" in optional else None)


def plan_red_unpack(n_streams, stream, seq, offsets, num_bytes, ring, ts_step, max_red=RED_MAX_DEPTH, timestamp=None, block_pt=None, optional=RED_UNPACK_OPTIONAL,
                    ring_capacity=None):
    """The rule of DecBatch.red_unpack on the host (lc3plus_plan_red_unpack, no device needed): the parse's items stream, seq, offsets (int64), num_bytes and the
    optional timestamp [n] over ring (uint8, ring_capacity bytes of it: all by default), optional block_pt [n_streams] -> dict of stream, seq, offsets (int64),
    num_bytes, timestamp, gen (uint8) [n * (max_red + 1)] - the item arrays of ingest and probe - status (uint8) [n] and stats [RED_UNPACK_STATS_WORDS]; those of
    RED_UNPACK_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    v = _red_unpack_arrays(n_streams, stream, seq, offsets, num_bytes, ring, ts_step, max_red, timestamp, block_pt, optional, ring_capacity)
    return _plan("lc3plus_plan_red_unpack", v, RED_UNPACK_OUTPUTS, n_streams=n_streams)


# ---- generic FEC ----
def fec_work_bytes(n_routes, n_frames):
    """bytes of the workspace of a fec_encode call (lc3plus_fec_work_bytes); 0 for arguments the calls refuse"""
    return int(_lib().lc3plus_fec_work_bytes(int(n_routes), int(n_frames)))


def fec_recover_work_bytes(n_streams, window):
    """bytes of the workspace of a fec_recover call (lc3plus_fec_recover_work_bytes); 0 for arguments the call refuses"""
    return int(_lib().lc3plus_fec_recover_work_bytes(int(n_streams), int(window)))


def _fec_encode_arrays(pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, fec_stride, header_room, payload_room,
                       fec_header_room, pkt_status, n_packets, route_stats, flush, state, acc, acc_stride, max_fec_packets, wire_capacity, fec_capacity, optional,
                       seq_in_place):
    """the values of an encode call by header parameter name: the arrays as the C calls take them (None for a NULL one; fec_wire a copy), the outputs and the
    workspace among them.  seq_in_place: next_fec_seq is the array fec_seq_base itself"""
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
    return dict(max_packets=m, n_packets=count, pkt_route=route, pkt_frame=frame, pkt_offset=offset, pkt_size=size, pkt_status=status, wire=wire,
                wire_capacity=wire.size if wire_capacity is None else wire_capacity, header_room=header_room, payload_room=payload_room, n_routes=R, n_frames=n_frames,
                seq_base=seq_base, route_stats=route_stats, group=group, flush=flush, fec_seq_base=fec_seq_base, state_in=state, acc_in=acc, state_out=state_out,
                acc_out=acc_out, acc_stride=acc_stride or 0, fec_wire=fec_wire, fec_capacity=fec_wire.size if fec_capacity is None else fec_capacity,
                fec_stride=fec_stride, fec_header_room=fec_header_room, max_fec_packets=q, n_fec=np.zeros(1, np.int64), fec_route=np.zeros(n, np.int32),
                fec_seq=np.zeros(n, np.int32), fec_frame=np.zeros(n, np.int32), fec_offset=np.zeros(n, np.int64), fec_size=np.zeros(n, np.int32),
                fec_flags=np.zeros(n, np.uint8) if "fec_flags" in optional else None, fec_mask=np.zeros(n, np.int32) if "fec_mask" in optional else None,
                next_fec_seq=fec_seq_base if seq_in_place else np.zeros(R, np.int32) if "next_fec_seq" in optional else None,
                route_stats_out=np.zeros((R, FEC_ROUTE_STATS_WORDS), np.int32) if "route_stats" in optional else None,
                work=np.zeros(max(fec_work_bytes(R, n_frames), 8) // 8, np.int64))


def _poison(v, byte):
    """poison_work of the conveniences: the workspace filled with a byte before the call (its contents mean nothing)"""
    if byte is not None:
        v["work"].view(np.uint8)[:] = int(byte)
    return v


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
    v = _fec_encode_arrays(pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, fec_stride, header_room, payload_room,
                           fec_header_room, pkt_status, n_packets, route_stats, flush, state, acc, acc_stride, max_fec_packets, wire_capacity, fec_capacity, optional,
                           seq_in_place)
    return _plan("lc3plus_plan_fec_encode", v, FEC_ENCODE_OUTPUTS, ("n_fec",))


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
        _device_call(self._ss + "_fec_encode", locals())

    def fec_encode(self, pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, fec_stride, header_room=12, payload_room=0,
                   fec_header_room=12, pkt_status=None, n_packets=None, route_stats=None, flush=None, state=None, acc=None, acc_stride=None, max_fec_packets=None,
                   wire_capacity=None, fec_capacity=None, optional=FEC_ENCODE_OPTIONAL, poison_work=None, seq_in_place=False):
        """Host convenience: the arrays of plan_fec_encode uploaded, encoded on the device and downloaded -> the dict plan_fec_encode gives.  Device memory through
        the HIP runtime (on the current device: the batch's, unless the caller has switched), freed before it returns.  poison_work: a byte the workspace is
        filled with before the call (its contents mean nothing); seq_in_place as in plan_fec_encode."""
        v = _fec_encode_arrays(pkt_route, pkt_frame, pkt_offset, pkt_size, wire, n_frames, seq_base, group, fec_seq_base, fec_wire, fec_stride, header_room,
                               payload_room, fec_header_room, pkt_status, n_packets, route_stats, flush, state, acc, acc_stride, max_fec_packets, wire_capacity,
                               fec_capacity, optional, seq_in_place)
        return _run(self, self._ss + "_fec_encode", _poison(v, poison_work), FEC_ENCODE_OUTPUTS, ("n_fec",))


def _fec_recover_arrays(n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, rec_offset, rec_stride, window, ring_capacity,
                        optional):
    """the values of a recover call by header parameter name: the arrays as the C calls take them (None for a NULL one; ring a copy), the outputs and the workspace
    among them"""
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
    return dict(n_items=n, ring=ring, ring_capacity=ring.size if ring_capacity is None else ring_capacity, dg_offsets=dg_offsets, dg_sizes=dg_sizes, stream=stream,
                seq=seq, n_fec=m, fec_stream=fec_stream, fec_offsets=fec_offsets, fec_num_bytes=fec_num_bytes, window=window, ssrc=ssrc, rec_offset=rec_offset,
                rec_stride=rec_stride, rec_dg_offsets=np.zeros(m, np.int64), rec_dg_sizes=np.zeros(m, np.int32), rec_seq=np.zeros(m, np.int32),
                status=np.zeros(m, np.uint8) if "status" in optional else None, stats=np.zeros(FEC_STATS_WORDS, np.int32) if "stats" in optional else None,
                work=np.zeros(max(fec_recover_work_bytes(n_streams, window), 8) // 8, np.int64))


def plan_fec_recover(n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, rec_offset, rec_stride, window=1024,
                     ring_capacity=None, optional=FEC_RECOVER_OPTIONAL):
    """The rule of DecBatch.fec_recover on the host (lc3plus_plan_fec_recover, no device needed): the datagrams dg_offsets (int64), dg_sizes with the media parse's
    stream, seq [n_items], the FEC parse's items fec_stream, fec_offsets (int64), fec_num_bytes [n_fec] over ring (uint8, its contents before the call), ssrc
    [n_streams] -> dict of ring (after the call: recovered packets at rec_offset + f * rec_stride), rec_dg_offsets (int64), rec_dg_sizes, rec_seq, status (uint8)
    [n_fec] and stats [FEC_STATS_WORDS]; those of FEC_RECOVER_OPTIONAL not named in `optional` are passed as NULL and come back as None.  LC3Error for arguments
    the C call refuses."""
    v = _fec_recover_arrays(n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, rec_offset, rec_stride, window,
                            ring_capacity, optional)
    return _plan("lc3plus_plan_fec_recover", v, FEC_RECOVER_OUTPUTS, n_streams=n_streams)


def fec_repair_work_bytes(n_streams, med_slots, fec_slots):
    """bytes of the workspace of a fec_repair call (lc3plus_fec_repair_work_bytes); 0 for arguments the call refuses"""
    return int(_lib().lc3plus_fec_repair_work_bytes(int(n_streams), int(med_slots), int(fec_slots)))


def fec_repair_stores(n_streams, ring, med_offset, med_slots=16, med_stride=None, fec_slots=4, fec_stride=None):
    """The stores of a receiver that has received nothing, as plan_fec_repair and DecBatch.fec_repair take and return them: dict of ring (a copy), med_offset,
    med_slots, med_stride, fec_slots, fec_stride and the zeroed med_seq, med_size [n_streams, H], fec_store [n_streams, P, fec_stride], cell_seq, cell_size,
    cell_status [n_streams, P], state [n_streams, FEC_REPAIR_STATE_WORDS]"""
    n, H, P = int(n_streams), int(med_slots), int(fec_slots)
    return dict(ring=np.array(ring, dtype=np.uint8).reshape(-1), med_offset=int(med_offset), med_slots=H, med_stride=int(med_stride), fec_slots=P,
                fec_stride=int(fec_stride), med_seq=np.zeros((n, H), np.int32), med_size=np.zeros((n, H), np.int32), fec_store=np.zeros((n, P, int(fec_stride)), np.uint8),
                cell_seq=np.zeros((n, P), np.int32), cell_size=np.zeros((n, P), np.int32), cell_status=np.zeros((n, P), np.uint8),
                state=np.zeros((n, FEC_REPAIR_STATE_WORDS), np.int32))


def _fec_repair_arrays(n_streams, stores, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, fec_seq, ssrc, passes, ring_capacity, optional):
    """the values of a repair call by header parameter name: the item arrays as the C calls take them (None for those of an empty list), copies of the stores,
    which the call advances in place, the outputs and the workspace"""
    n, H, P = int(n_streams), int(stores["med_slots"]), int(stores["fec_slots"])
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
    m = stream.size
    fec_stream = np.ascontiguousarray(fec_stream, dtype=np.int32).reshape(-1)
    k = fec_stream.size
    per = lambda a, dt, size, what: _shaped(np.ascontiguousarray(a, dtype=dt).reshape(-1), (size,), what) if size else None
    media, fec = "the item arrays hold one entry per item", "the FEC item arrays hold one entry per FEC item"
    ring = np.array(stores["ring"], dtype=np.uint8).reshape(-1)
    v = dict(n_items=m, ring=ring, ring_capacity=ring.size if ring_capacity is None else ring_capacity, dg_offsets=per(dg_offsets, np.int64, m, media),
             dg_sizes=per(dg_sizes, np.int32, m, media), stream=stream if m else None, seq=_shaped(_u32(seq), (m,), media) if m else None, n_fec=k,
             fec_stream=fec_stream if k else None, fec_offsets=per(fec_offsets, np.int64, k, fec), fec_num_bytes=per(fec_num_bytes, np.int32, k, fec),
             fec_seq=_shaped(_u32(fec_seq), (k,), fec) if k else None, ssrc=_shaped(_u32(ssrc), (n,), "ssrc holds one entry per stream"),
             med_offset=stores["med_offset"], med_slots=H, med_stride=stores["med_stride"], fec_slots=P, fec_stride=stores["fec_stride"], passes=passes)
    for name, dt, shape in (("med_seq", np.int32, (n, H)), ("med_size", np.int32, (n, H)), ("fec_store", np.uint8, (n, P, int(stores["fec_stride"]))),
                            ("cell_seq", np.int32, (n, P)), ("cell_size", np.int32, (n, P)), ("cell_status", np.uint8, (n, P)),
                            ("state", np.int32, (n, FEC_REPAIR_STATE_WORDS))):
        v[name] = _shaped(np.array(stores[name], dtype=dt), shape, "%s must have shape %r" % (name, shape))
    v.update(rec_dg_offsets=np.zeros(n * P, np.int64), rec_dg_sizes=np.zeros(n * P, np.int32), rec_seq=np.zeros(n * P, np.int32),
             item_status=np.zeros(m, np.uint8) if "item_status" in optional else None, fec_status=np.zeros(k, np.uint8) if "fec_status" in optional else None,
             stats=np.zeros(FEC_STATS_WORDS, np.int32) if "stats" in optional else None,
             work=np.zeros(max(fec_repair_work_bytes(n, H, P), 8) // 8, np.int64))
    return v


def _fec_repair_result(v, stores):
    """the dict a repair gives: the outputs and the advanced stores, with the stores' shape parameters - so that it is the next call's `stores`"""
    r = _result(v, FEC_REPAIR_OUTPUTS)
    r.update({k: stores[k] for k in ("med_offset", "med_slots", "med_stride", "fec_slots", "fec_stride")})
    return r


def plan_fec_repair(n_streams, stores, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, fec_seq, ssrc, passes=1, ring_capacity=None,
                    optional=FEC_REPAIR_OPTIONAL, poison_work=None):
    """The rule of DecBatch.fec_repair on the host (lc3plus_plan_fec_repair, no device needed).  stores: fec_repair_stores(...) or the dict an earlier call gave,
    with this call's datagrams written into its ring; the media parse's dg_offsets (int64), dg_sizes, stream, seq [n_items] and the FEC parse's fec_stream,
    fec_offsets (int64), fec_num_bytes, fec_seq [n_fec] (either list may be empty), ssrc [n_streams] -> dict of the advanced stores (FEC_REPAIR_STORES, copies: the
    argument stays as it was) with their shape parameters, rec_dg_offsets (int64), rec_dg_sizes, rec_seq [n_streams * P], item_status (uint8) [n_items],
    fec_status (uint8) [n_fec] and stats [FEC_STATS_WORDS]; those of FEC_REPAIR_OPTIONAL not named in `optional` are passed as NULL and come back as None.  A test
    chains calls by passing the dict back.  LC3Error for arguments the C call refuses."""
    v = _fec_repair_arrays(n_streams, stores, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, fec_seq, ssrc, passes, ring_capacity, optional)
    _plan("lc3plus_plan_fec_repair", _poison(v, poison_work), (), n_streams=n_streams)
    return _fec_repair_result(v, stores)


# ---- reception reports ----
def rtcp_workspace_bytes(n_items, n_streams):
    """the bytes of the workspace a DecBatch.rtcp_stats_device call over n_items items and n_streams streams needs (lc3plus_rtcp_workspace_bytes); 0 for
    arguments the call refuses"""
    return int(_lib().lc3plus_rtcp_workspace_bytes(int(n_items), int(n_streams)))


def _rtcp_arrays(stream, seq, timestamp, arrival, state, make_report, ssrc, lsr, dlsr, optional):
    """the values of a stats call by header parameter name: the arrays as the C calls take them (None for a NULL one), the outputs among them"""
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
    n = stream.size
    seq, timestamp, arrival = _u32(seq), _u32(timestamp), _u32(arrival)
    if not (seq.size == timestamp.size == arrival.size == n):
        raise ValueError("stream, seq, timestamp and arrival hold one entry per item")
    state = _u32(state).reshape(-1, RR_STATE_WORDS) if np.asarray(state).size % RR_STATE_WORDS == 0 else None
    if state is None:
        raise ValueError("state must have shape [n_streams, RR_STATE_WORDS]")
    S = state.shape[0]
    ssrc, lsr, dlsr = [None if a is None else _u32(a) for a in (ssrc, lsr, dlsr)]
    if any(a is not None and a.size != S for a in (ssrc, lsr, dlsr)):
        raise ValueError("ssrc, lsr and dlsr hold one entry per stream")
    return dict(n_items=n, stream=stream, seq=seq, timestamp=timestamp, arrival=arrival, n_streams=S, state_in=np.ascontiguousarray(state),
                state_out=np.zeros((S, RR_STATE_WORDS), np.int32), make_report=make_report, ssrc=ssrc, lsr=lsr, dlsr=dlsr,
                blocks=np.zeros((S, RR_BLOCK_BYTES), np.uint8) if make_report else None, ext_seq=np.zeros(n, np.int32) if "ext_seq" in optional else None,
                item_status=np.zeros(n, np.uint8) if "item_status" in optional else None,
                stream_stats=np.zeros((S, RR_STATS_WORDS), np.int32) if "stream_stats" in optional else None)


def plan_rtcp_stats(stream, seq, timestamp, arrival, state, make_report=False, ssrc=None, lsr=None, dlsr=None, optional=RR_OPTIONAL):
    """The rule of DecBatch.rtcp_stats on the host (lc3plus_plan_rtcp_stats, no device needed): the parse's item arrays stream / seq / timestamp [n] and the
    arrival time of each item on its stream's RTP clock, state [n_streams, RR_STATE_WORDS] (zeros: a source that has not started), with make_report ssrc and
    optionally lsr, dlsr [n_streams] -> dict of state (the advanced state), blocks [n_streams, RR_BLOCK_BYTES] (uint8; None without make_report), ext_seq [n],
    item_status (uint8) [n] and stream_stats [n_streams, RR_STATS_WORDS]; those of RR_OPTIONAL not named in `optional` are passed as NULL and come back as
    None.  LC3Error for arguments the C call refuses."""
    v = _rtcp_arrays(stream, seq, timestamp, arrival, state, make_report, ssrc, lsr, dlsr, optional)
    return _plan("lc3plus_plan_rtcp_stats", v, RR_OUTPUTS, make_report=1 if make_report else 0)          # any true value; the batch call takes the number itself


# ---- Secure RTP ----
def srtp_make_context(master_key, master_salt):
    """An SRTP crypto context (lc3plus_srtp_make_context, host only): master_key (16 bytes) and master_salt (14 bytes) -> SRTP_CTX_WORDS int32 words - the
    round keys of the session cipher key, the session salt and the two SHA-1 midstates of the HMAC under the session authentication key (RFC 3711 4.3.1,
    key derivation rate 0) - as the device reads them; the caller stacks contexts into [n, SRTP_CTX_WORDS] and copies them to device memory."""
    key, salt = np.frombuffer(bytes(master_key), np.uint8), np.frombuffer(bytes(master_salt), np.uint8)
    if key.size != 16 or salt.size != 14:
        raise ValueError("master_key holds 16 bytes, master_salt 14")
    ctx = np.zeros(SRTP_CTX_WORDS, np.int32)
    _check(_lib().lc3plus_srtp_make_context(key.ctypes.data, salt.ctypes.data, ctx.ctypes.data), "lc3plus_srtp_make_context")
    return ctx


def srtp_gcm_make_context(master_key, master_salt):
    """An SRTP AES-GCM crypto context (lc3plus_srtp_gcm_make_context, host only): master_key (16 bytes: AEAD_AES_128_GCM; 32 bytes: AEAD_AES_256_GCM) and
    master_salt (12 bytes) -> SRTP_GCM_CTX_WORDS int32 words - the round keys of the session key, the number of rounds, the session salt and the GHASH table
    (RFC 7714 11, key derivation rate 0) - as the device reads them; the caller stacks contexts, of both key sizes where it likes, into
    [n, SRTP_GCM_CTX_WORDS] and copies them to device memory."""
    key, salt = np.frombuffer(bytes(master_key), np.uint8), np.frombuffer(bytes(master_salt), np.uint8)
    if key.size not in (16, 32) or salt.size != 12:
        raise ValueError("master_key holds 16 or 32 bytes, master_salt 12")
    ctx = np.zeros(SRTP_GCM_CTX_WORDS, np.int32)
    _check(_lib().lc3plus_srtp_gcm_make_context(key.ctypes.data, key.size, salt.ctypes.data, ctx.ctypes.data), "lc3plus_srtp_gcm_make_context")
    return ctx


def srtp_workspace_bytes(n_items, n_ssrc):
    """the bytes of the workspace a DecBatch.srtp_unprotect_device call over n_items datagrams and n_ssrc sources needs (lc3plus_srtp_workspace_bytes); 0 for
    arguments the call refuses"""
    return int(_lib().lc3plus_srtp_workspace_bytes(int(n_items), int(n_ssrc)))


# a Secure RTP suite as the calls below take it, the infix of its C symbols: the words of its context (the AEAD suites' symbols take no tag_len: PARAMS)
_SRTP_CTX_WORDS = {"srtp": SRTP_CTX_WORDS, "srtp_gcm": SRTP_GCM_CTX_WORDS}


def _plan_srtp_protect(suite, pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, tag_len, header_room, payload_room, next_seq,
                       n_packets, wire_capacity, dst_capacity):
    route = np.ascontiguousarray(pkt_route, dtype=np.int32).reshape(-1)
    m = route.size
    off, size = np.ascontiguousarray(pkt_offset, dtype=np.int64).reshape(-1), np.ascontiguousarray(pkt_size, dtype=np.int32).reshape(-1)
    pst = np.ascontiguousarray(pkt_status, dtype=np.uint8).reshape(-1)
    if not (off.size == size.size == pst.size == m):
        raise ValueError("the list arrays hold one entry per packet")
    ctx = np.ascontiguousarray(_u32(ctx)).reshape(-1, _SRTP_CTX_WORDS[suite])
    R = ctx.shape[0]
    roc, seq_base = _u32(roc), _u32(seq_base)
    next_seq = _u32(next_seq) if next_seq is not None else None
    if roc.size != R or seq_base.size != R or (next_seq is not None and next_seq.size != R):
        raise ValueError("ctx, roc, seq_base and next_seq hold one entry per route")
    wire = np.ascontiguousarray(wire, dtype=np.uint8).reshape(-1)
    dst = np.array(dst, dtype=np.uint8).reshape(-1)                   # a copy: the call's destination starts with these contents
    count = np.array([m if n_packets is None else int(n_packets)], np.int64)
    v = dict(max_packets=m, n_packets=count, pkt_route=route, pkt_offset=off, pkt_size=size, pkt_status=pst, wire=wire,
             wire_capacity=wire.size if wire_capacity is None else wire_capacity, header_room=header_room, payload_room=payload_room, n_routes=R, ctx=ctx, roc=roc,
             seq_base=seq_base, next_seq=next_seq, dst=dst, dst_capacity=dst.size if dst_capacity is None else dst_capacity, dst_stride=dst_stride, tag_len=tag_len,
             out_offset=np.zeros(m, np.int64), out_size=np.zeros(m, np.int32), out_status=np.zeros(m, np.uint8),
             next_roc=np.zeros(R, np.int32) if next_seq is not None else None)
    return _plan("lc3plus_plan_%s_protect" % suite, v, SRTP_PROTECT_OUTPUTS + ("dst",))


def plan_srtp_protect(pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, tag_len=10, header_room=12, payload_room=0,
                      next_seq=None, n_packets=None, wire_capacity=None, dst_capacity=None):
    """The rule of Batch.srtp_protect_device / DecBatch.srtp_protect_device on the host (lc3plus_plan_srtp_protect, no device needed): the stamp's view of the
    egress's packet list pkt_route, pkt_offset (int64), pkt_size, pkt_status (uint8) [max_packets] (n_packets of it: all by default), the stamped wire buffer
    (uint8; wire_capacity bytes of it), per route ctx [n_routes, SRTP_CTX_WORDS], roc, seq_base and optionally next_seq [n_routes]; dst: the destination's
    contents before the call (uint8; dst_capacity bytes of it) -> dict of dst (the buffer after the call), out_offset (int64), out_size, out_status (uint8)
    [max_packets] (zero behind n_packets) and next_roc [n_routes] (None without next_seq).  LC3Error for arguments the C call refuses."""
    return _plan_srtp_protect("srtp", pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, tag_len, header_room, payload_room,
                              next_seq, n_packets, wire_capacity, dst_capacity)


def plan_srtp_gcm_protect(pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, header_room=12, payload_room=0, next_seq=None,
                          n_packets=None, wire_capacity=None, dst_capacity=None):
    """plan_srtp_protect for the AEAD suites (lc3plus_plan_srtp_gcm_protect): the same arguments without tag_len, ctx [n_routes, SRTP_GCM_CTX_WORDS] -> the same
    dict; a protected packet is SRTP_GCM_TAG_BYTES longer than its RTP packet."""
    return _plan_srtp_protect("srtp_gcm", pkt_route, pkt_offset, pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, dst_stride, None, header_room, payload_room,
                              next_seq, n_packets, wire_capacity, dst_capacity)


_SRTP_UNPROTECT_RESULT = SRTP_UNPROTECT_OUTPUTS + ("ring",)


def _srtp_unprotect_arrays(suite, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity):
    """the values of an unprotect call by header parameter name: the arrays as the C calls take them (None for a NULL one; ring a copy), the outputs among them"""
    ring, dg_offsets = np.array(ring, dtype=np.uint8).reshape(-1), np.ascontiguousarray(dg_offsets, dtype=np.int64).reshape(-1)
    dg_sizes, ssrc_key = np.ascontiguousarray(dg_sizes, dtype=np.int32).reshape(-1), _u32(ssrc_key)
    ctx, state = np.ascontiguousarray(_u32(ctx)).reshape(-1, _SRTP_CTX_WORDS[suite]), np.ascontiguousarray(_u32(state)).reshape(-1, SRTP_STATE_WORDS)
    n, n_ssrc = dg_offsets.size, ssrc_key.size
    if n != dg_sizes.size:
        raise ValueError("dg_offsets and dg_sizes hold one entry per datagram")
    if ctx.shape[0] != n_ssrc or state.shape[0] != n_ssrc:
        raise ValueError("ssrc_key, ctx and state hold one entry per source")
    return dict(n_items=n, ring=ring, ring_capacity=ring.size if ring_capacity is None else ring_capacity, dg_offsets=dg_offsets, dg_sizes=dg_sizes, n_ssrc=n_ssrc,
                ssrc_key=ssrc_key, ctx=ctx, state_in=state, state_out=np.zeros((n_ssrc, SRTP_STATE_WORDS), np.int32), tag_len=tag_len, sizes_out=np.zeros(n, np.int32),
                status=np.zeros(n, np.uint8) if "status" in optional else None, index=np.zeros(n, np.int64) if "index" in optional else None,
                stats=np.zeros(SRTP_STATS_WORDS, np.int32) if "stats" in optional else None)


def plan_srtp_unprotect(ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len=10, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
    """The rule of DecBatch.srtp_unprotect on the host (lc3plus_plan_srtp_unprotect, no device needed): ring (uint8, ring_capacity bytes of it: all by default),
    the datagrams dg_offsets (int64) / dg_sizes [n], the sources ssrc_key (ascending as uint32) with ctx [n_ssrc, SRTP_CTX_WORDS] and state [n_ssrc,
    SRTP_STATE_WORDS] (zeros: a source that has not started) -> dict of ring (the buffer after the call: accepted payloads decrypted), state (the advanced
    state), sizes [n] (rtp_parse's dg_sizes), status (uint8) [n], index (int64) [n] and stats [SRTP_STATS_WORDS]; those of SRTP_UNPROTECT_OPTIONAL not named in
    `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    v = _srtp_unprotect_arrays("srtp", ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity)
    return _plan("lc3plus_plan_srtp_unprotect", v, _SRTP_UNPROTECT_RESULT)


def plan_srtp_gcm_unprotect(ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
    """plan_srtp_unprotect for the AEAD suites (lc3plus_plan_srtp_gcm_unprotect): the same arguments without tag_len, ctx [n_ssrc, SRTP_GCM_CTX_WORDS] -> the
    same dict."""
    v = _srtp_unprotect_arrays("srtp_gcm", ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, None, optional, ring_capacity)
    return _plan("lc3plus_plan_srtp_gcm_unprotect", v, _SRTP_UNPROTECT_RESULT)


class _SrtpProtect:
    """The send side of Secure RTP for both batch kinds (lc3plus_{enc,dec}_batch_srtp_protect and _srtp_gcm_protect; include/lc3plus_batch.h "Secure RTP")."""

    def srtp_protect_device(self, max_packets, d_n_packets_ptr, d_pkt_route_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, d_pkt_status_ptr, d_wire_ptr, wire_capacity,
                            n_routes, d_ctx_ptr, d_roc_ptr, d_seq_base_ptr, d_dst_ptr, dst_capacity, dst_stride, d_out_offset_ptr, d_out_size_ptr,
                            d_out_status_ptr, tag_len=10, header_room=12, payload_room=0, d_next_seq_ptr=None, d_next_roc_ptr=None, hip_stream=None, sync=False):
        """Raw device pointers only - the egress's packet list as rtp_stamp_device took it with the stamp's pkt_status, the stamped wire buffer, per route ctx
        [n_routes, SRTP_CTX_WORDS], roc, seq_base and optionally next_seq -> every stamped packet as an SRTP packet (header, encrypted payload, tag of tag_len
        bytes) at dst + p * dst_stride, out_offset (int64), out_size, out_status (uint8) [max_packets] and the optional next_roc [n_routes].  Stateless: nothing
        of the batch's streams is read or written.  Queued on hip_stream; returns at once unless sync."""
        _device_call(self._ss + "_srtp_protect", locals())

    def srtp_gcm_protect_device(self, max_packets, d_n_packets_ptr, d_pkt_route_ptr, d_pkt_offset_ptr, d_pkt_size_ptr, d_pkt_status_ptr, d_wire_ptr, wire_capacity,
                                n_routes, d_ctx_ptr, d_roc_ptr, d_seq_base_ptr, d_dst_ptr, dst_capacity, dst_stride, d_out_offset_ptr, d_out_size_ptr,
                                d_out_status_ptr, header_room=12, payload_room=0, d_next_seq_ptr=None, d_next_roc_ptr=None, hip_stream=None, sync=False):
        """srtp_protect_device for the AEAD suites (lc3plus_{enc,dec}_batch_srtp_gcm_protect): the same arguments without tag_len, ctx [n_routes,
        SRTP_GCM_CTX_WORDS], routes of 16- and 32-byte keys side by side -> header, AES-GCM ciphertext and a tag of SRTP_GCM_TAG_BYTES bytes at
        dst + p * dst_stride."""
        _device_call(self._ss + "_srtp_gcm_protect", locals())


# ---- the receive side: the decoder batch alone ----
def _ingest_arrays(n_streams, channels, stream, seq, offsets, num_bytes, base, n_frames, seq_bits, info, floor, optional):
    """the values of an ingest call by header parameter name: the arrays as the C calls take them (None for a NULL one), the outputs among them"""
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
    n = stream.size
    seq, base = _u32(seq), _u32(base)
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
    return dict(n_items=n, stream=stream, seq=seq, offsets=offsets, num_bytes=num_bytes, info=info, base=base, floor=floor, seq_bits=seq_bits, n_frames=n_frames,
                out_offsets=np.zeros(cells, np.int64), out_num_bytes=np.zeros(cells, np.int32), cell_item=np.zeros(cells, np.int32), counts=np.zeros(cells[0], np.int32),
                next_base=np.zeros(cells[0], np.int32) if "next_base" in optional else None,
                stats=np.zeros((cells[0], ING_STATS_WORDS), np.int32) if "stats" in optional else None,
                item_status=np.zeros(n, np.uint8) if "item_status" in optional else None)


def plan_ingest(n_streams, channels, stream, seq, offsets, num_bytes, base, n_frames, seq_bits=16, info=None, floor=None, optional=ING_OPTIONAL):
    """The rule of DecBatch.ingest on the host (lc3plus_plan_ingest, no device needed): the item list stream / seq / offsets / num_bytes [n], base [n_streams],
    optional probe records info [n, channels, FRAME_INFO_WORDS] and floor [n_streams] -> dict of offsets (int64), num_bytes, cell_item [n_streams, n_frames],
    counts, next_base [n_streams], stats [n_streams, ING_STATS_WORDS] and item_status [n] (uint8); those of next_base, stats and item_status not named in
    `optional` are passed as NULL and come back as None.  LC3Error for arguments the C call refuses."""
    v = _ingest_arrays(n_streams, channels, stream, seq, offsets, num_bytes, base, n_frames, seq_bits, info, floor, optional)
    # to this plan alone an empty array is a NULL pointer, as it always was: an empty list is refused as a missing one is
    _plan("lc3plus_plan_ingest", {k: None if isinstance(a, np.ndarray) and not a.size else a for k, a in v.items()}, (), n_streams=n_streams, channels=channels)
    return _result(v, ING_OUTPUTS)


class _Receive:
    """The receive side of the packet layer, the decoder batch's alone: the frame probe, packet ingest, RTP parse, RED unpack, FEC recovery, reception reports and
    SRTP unprotect (lc3plus_dec_batch_*; include/lc3plus_batch.h)."""

    def probe_device(self, d_frames_ptr, frames_capacity, d_offsets_ptr, d_num_bytes_ptr, max_frame_bytes, n_items, d_info_ptr, depth=PROBE_FULL,
                     hip_stream=None, sync=False):
        """The frame probe (lc3plus_dec_batch_probe): raw device pointers only - frames frames_capacity bytes, offsets [n_items] int64, num_bytes [n_items]
        int32, info [n_items, channels, FRAME_INFO_WORDS] int32.  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns
        at once unless sync."""
        _device_call("lc3plus_dec_batch_probe", locals())

    def probe(self, payloads, depth=PROBE_FULL):
        """Host convenience: a list of stream-frames (bytes or uint8 arrays, all channels; empty = lost) packed back to back, uploaded, probed ->
        int32 [n, channels, FRAME_INFO_WORDS].  Device memory through the HIP runtime (hipMalloc / hipMemcpy on the current device: the batch's, unless the
        caller has switched), freed before it returns."""
        pl = [np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
              for x in payloads]
        nb = np.array([x.size for x in pl], np.int32)
        offs = (np.cumsum(nb, dtype=np.int64) - nb).astype(np.int64)
        buf = np.concatenate(pl + [np.zeros(4, np.uint8)])            # (never empty)
        v = dict(frames=buf, frames_capacity=buf.size - 4, offsets=offs, num_bytes=nb, max_frame_bytes=max(int(nb.max()), 1), n_items=len(pl), depth=depth,
                 info=np.zeros((len(pl), self.channels, FRAME_INFO_WORDS), np.int32))
        return _run(self, "lc3plus_dec_batch_probe", v, ("info",))["info"]

    def ingest_device(self, n_items, d_stream_ptr, d_seq_ptr, d_offsets_ptr, d_num_bytes_ptr, d_base_ptr, n_frames, d_out_offsets_ptr, d_out_num_bytes_ptr,
                      d_cell_item_ptr, d_counts_ptr, seq_bits=16, d_info_ptr=None, d_floor_ptr=None, d_next_base_ptr=None, d_stats_ptr=None,
                      d_item_status_ptr=None, hip_stream=None, sync=False):
        """Packet ingest (lc3plus_dec_batch_ingest): raw device pointers only - the item list stream, seq, num_bytes [n_items] int32 and offsets [n_items]
        int64, optional probe records info [n_items, channels, FRAME_INFO_WORDS], base and optional floor [n_streams] int32 -> out_offsets (int64),
        out_num_bytes, cell_item [n_streams, n_frames], counts [n_streams] and the optional next_base [n_streams], stats [n_streams, ING_STATS_WORDS] and
        item_status [n_items] uint8.  The tables are what decode_device_packed and set_frame_counts take.  Stateless: nothing of the batch's streams is read
        or written.  Queued on hip_stream; returns at once unless sync."""
        _device_call("lc3plus_dec_batch_ingest", locals())

    def ingest(self, stream, seq, offsets, num_bytes, base, n_frames, seq_bits=16, info=None, floor=None, optional=ING_OPTIONAL):
        """Host convenience: the arrays of plan_ingest uploaded, ingested on the device and downloaded -> the dict plan_ingest gives.  Device memory through the
        HIP runtime as in probe(), freed before it returns."""
        v = _ingest_arrays(self.n_streams, self.channels, stream, seq, offsets, num_bytes, base, n_frames, seq_bits, info, floor, optional)
        return _run(self, "lc3plus_dec_batch_ingest", v, ING_OUTPUTS)

    def rtp_parse_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, n_ssrc, d_ssrc_key_ptr, d_ssrc_stream_ptr, d_stream_ptr,
                         d_seq_ptr, d_offsets_ptr, d_num_bytes_ptr, d_payload_type_ptr=None, payload_room=0, d_timestamp_ptr=None, d_marker_ptr=None,
                         d_status_ptr=None, d_stats_ptr=None, hip_stream=None, sync=False):
        """The receive side of the RTP framing (lc3plus_dec_batch_rtp_parse): raw device pointers only - the datagrams dg_offsets (int64) / dg_sizes [n_items] in
        ring, the senders ssrc_key (ascending as uint32) / ssrc_stream [n_ssrc], optional payload_type [n_streams] -> stream, seq, offsets (int64), num_bytes
        [n_items], as ingest_device and probe_device take them (frames = ring, seq_bits = 16), and the optional timestamp [n_items], marker, status (uint8)
        [n_items] and stats [RTP_STATS_WORDS].  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns at once unless
        sync."""
        _device_call("lc3plus_dec_batch_rtp_parse", locals())

    def rtp_parse(self, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type=None, payload_room=0, optional=RTP_PARSE_OPTIONAL, ring_capacity=None):
        """Host convenience: the arrays of plan_rtp_parse uploaded, parsed on the device and downloaded -> the dict plan_rtp_parse gives.  Device memory through
        the HIP runtime as in probe(), freed before it returns."""
        v = _rtp_parse_arrays(self.n_streams, ring, dg_offsets, dg_sizes, ssrc_key, ssrc_stream, payload_type, payload_room, optional, ring_capacity)
        return _run(self, "lc3plus_dec_batch_rtp_parse", v, RTP_PARSE_OUTPUTS)

    def red_unpack_device(self, n_items, d_stream_ptr, d_seq_ptr, d_offsets_ptr, d_num_bytes_ptr, d_ring_ptr, ring_capacity, max_red, ts_step, d_out_stream_ptr,
                          d_out_seq_ptr, d_out_offsets_ptr, d_out_num_bytes_ptr, d_timestamp_ptr=None, d_block_pt_ptr=None, d_out_timestamp_ptr=None,
                          d_out_gen_ptr=None, d_status_ptr=None, d_stats_ptr=None, hip_stream=None, sync=False):
        """The receive side of the redundant audio (lc3plus_dec_batch_red_unpack): raw device pointers only - rtp_parse_device's stream, seq, offsets (int64),
        num_bytes and optional timestamp [n_items] as they stand, over its ring, optional block_pt [n_streams] -> out_stream, out_seq, out_offsets (int64),
        out_num_bytes [n_items * (max_red + 1)], as ingest_device and probe_device take them, and the optional out_timestamp, out_gen (uint8) of that length,
        status (uint8) [n_items] and stats [RED_UNPACK_STATS_WORDS].  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns
        at once unless sync."""
        _device_call("lc3plus_dec_batch_red_unpack", locals())

    def red_unpack(self, stream, seq, offsets, num_bytes, ring, ts_step, max_red=RED_MAX_DEPTH, timestamp=None, block_pt=None, optional=RED_UNPACK_OPTIONAL,
                   ring_capacity=None):
        """Host convenience: the arrays of plan_red_unpack uploaded, unpacked on the device and downloaded -> the dict plan_red_unpack gives.  Device memory
        through the HIP runtime as in probe(), freed before it returns."""
        v = _red_unpack_arrays(self.n_streams, stream, seq, offsets, num_bytes, ring, ts_step, max_red, timestamp, block_pt, optional, ring_capacity)
        return _run(self, "lc3plus_dec_batch_red_unpack", v, RED_UNPACK_OUTPUTS)

    def fec_recover_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, d_stream_ptr, d_seq_ptr, n_fec, d_fec_stream_ptr, d_fec_offsets_ptr,
                           d_fec_num_bytes_ptr, window, d_ssrc_ptr, rec_offset, rec_stride, d_rec_dg_offsets_ptr, d_rec_dg_sizes_ptr, d_rec_seq_ptr, d_work_ptr,
                           d_status_ptr=None, d_stats_ptr=None, hip_stream=None, sync=False):
        """The receive side of the generic FEC (lc3plus_dec_batch_fec_recover): raw device pointers only - the datagram list dg_offsets (int64), dg_sizes with the
        media parse's stream, seq [n_items], the FEC parse's fec_stream, fec_offsets (int64), fec_num_bytes [n_fec] over the ring, ssrc [n_streams] -> every media
        packet that is the only one missing of an FEC item's group rebuilt at ring + rec_offset + f * rec_stride, and rec_dg_offsets (int64), rec_dg_sizes,
        rec_seq [n_fec] - a datagram list for rtp_parse_device - with the optional status (uint8) [n_fec] and stats [FEC_STATS_WORDS].  work:
        fec_recover_work_bytes(n_streams, window) bytes.  Stateless: nothing of the batch's streams is read or written.  Queued on hip_stream; returns at once
        unless sync."""
        _device_call("lc3plus_dec_batch_fec_recover", locals())

    def fec_recover(self, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, rec_offset, rec_stride, window=1024, ring_capacity=None,
                    optional=FEC_RECOVER_OPTIONAL, poison_work=None):
        """Host convenience: the arrays of plan_fec_recover uploaded, recovered on the device and downloaded -> the dict plan_fec_recover gives.  Device memory
        through the HIP runtime as in probe(), freed before it returns.  poison_work: a byte the workspace is filled with before the call."""
        v = _fec_recover_arrays(self.n_streams, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc, rec_offset, rec_stride, window,
                                ring_capacity, optional)
        return _run(self, "lc3plus_dec_batch_fec_recover", _poison(v, poison_work), FEC_RECOVER_OUTPUTS)

    def fec_repair_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, d_stream_ptr, d_seq_ptr, n_fec, d_fec_stream_ptr, d_fec_offsets_ptr,
                          d_fec_num_bytes_ptr, d_fec_seq_ptr, d_ssrc_ptr, med_offset, med_slots, med_stride, d_med_seq_ptr, d_med_size_ptr, d_fec_store_ptr, fec_slots,
                          fec_stride, d_cell_seq_ptr, d_cell_size_ptr, d_cell_status_ptr, d_state_ptr, d_rec_dg_offsets_ptr, d_rec_dg_sizes_ptr, d_rec_seq_ptr,
                          d_work_ptr, passes=1, d_item_status_ptr=None, d_fec_status_ptr=None, d_stats_ptr=None, hip_stream=None, sync=False):
        """Generic FEC across calls (lc3plus_dec_batch_fec_repair): raw device pointers only - this call's media items dg_offsets (int64), dg_sizes, stream, seq
        [n_items] and FEC items fec_stream, fec_offsets (int64), fec_num_bytes, fec_seq [n_fec] over the ring (either list may be empty, its pointers then 0),
        ssrc [n_streams], and the caller's stores, advanced in place: the media history inside the ring (med_offset, med_slots, med_stride) with med_seq, med_size
        [n_streams, H], fec_store [n_streams, P, fec_stride] with cell_seq, cell_size, cell_status (uint8) [n_streams, P], state [n_streams,
        FEC_REPAIR_STATE_WORDS] -> the arrivals admitted, up to `passes` recovery passes run, rebuilt packets in their media slots and listed in rec_dg_offsets
        (int64), rec_dg_sizes, rec_seq [n_streams * P] - a datagram list for rtp_parse_device - with the optional item_status (uint8) [n_items], fec_status (uint8)
        [n_fec] and stats [FEC_STATS_WORDS].  work: fec_repair_work_bytes(n_streams, med_slots, fec_slots) bytes.  Nothing of the batch's streams is read or
        written.  Queued on hip_stream; returns at once unless sync."""
        _device_call("lc3plus_dec_batch_fec_repair", locals())

    def fec_repair(self, stores, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, fec_seq, ssrc, passes=1, ring_capacity=None,
                   optional=FEC_REPAIR_OPTIONAL, poison_work=None):
        """Host convenience: the arrays of plan_fec_repair uploaded, repaired on the device and downloaded -> the dict plan_fec_repair gives, the advanced stores
        in it, so that a caller chains calls by passing it back.  Device memory through the HIP runtime as in probe(), freed before it returns.  poison_work: a
        byte the workspace is filled with before the call."""
        v = _fec_repair_arrays(self.n_streams, stores, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, fec_seq, ssrc, passes, ring_capacity,
                               optional)
        _run(self, "lc3plus_dec_batch_fec_repair", _poison(v, poison_work), FEC_REPAIR_OUTPUTS)
        return _fec_repair_result(v, stores)

    def rtcp_stats_device(self, n_items, d_stream_ptr, d_seq_ptr, d_timestamp_ptr, d_arrival_ptr, n_streams, d_state_in_ptr, d_state_out_ptr, d_workspace_ptr,
                          workspace_bytes, make_report=False, d_ssrc_ptr=None, d_lsr_ptr=None, d_dlsr_ptr=None, d_blocks_ptr=None, d_ext_seq_ptr=None,
                          d_item_status_ptr=None, d_stream_stats_ptr=None, hip_stream=None, sync=False):
        """Reception reports (lc3plus_dec_batch_rtcp_stats): raw device pointers only - rtp_parse_device's stream, seq and timestamp [n_items] as they stand, the
        arrival time of each item, state_in / state_out [n_streams, RR_STATE_WORDS] (they may be one array), a workspace of rtcp_workspace_bytes(n_items,
        n_streams) bytes -> the advanced state, with make_report the report blocks [n_streams, RR_BLOCK_BYTES] (needs ssrc; lsr, dlsr optional), and the optional
        ext_seq [n_items], item_status (uint8) [n_items] and stream_stats [n_streams, RR_STATS_WORDS].  Stateless: nothing of the batch's streams is read or
        written.  Queued on hip_stream; returns at once unless sync."""
        _device_call("lc3plus_dec_batch_rtcp_stats", locals())          # make_report as the number it is: True is 1

    def rtcp_stats(self, stream, seq, timestamp, arrival, state, make_report=False, ssrc=None, lsr=None, dlsr=None, optional=RR_OPTIONAL):
        """Host convenience: the arrays of plan_rtcp_stats uploaded, run on the device and downloaded -> the dict plan_rtcp_stats gives.  Device memory through
        the HIP runtime as in probe(), the workspace too, freed before it returns."""
        v = _rtcp_arrays(stream, seq, timestamp, arrival, state, make_report, ssrc, lsr, dlsr, optional)
        work = np.zeros(max(rtcp_workspace_bytes(v["n_items"], v["n_streams"]), 8), np.uint8)
        return _run(self, "lc3plus_dec_batch_rtcp_stats", dict(v, workspace=work, workspace_bytes=work.size), RR_OUTPUTS)

    def _srtp_unprotect(self, suite, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity):
        v = _srtp_unprotect_arrays(suite, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity)
        work = np.zeros(max(srtp_workspace_bytes(v["n_items"], v["n_ssrc"]), 8), np.uint8)
        return _run(self, "lc3plus_dec_batch_%s_unprotect" % suite, dict(v, workspace=work, workspace_bytes=work.size), _SRTP_UNPROTECT_RESULT)

    def srtp_unprotect_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, n_ssrc, d_ssrc_key_ptr, d_ctx_ptr, d_state_in_ptr,
                              d_state_out_ptr, d_sizes_out_ptr, d_workspace_ptr, workspace_bytes, tag_len=10, d_status_ptr=None, d_index_ptr=None, d_stats_ptr=None,
                              hip_stream=None, sync=False):
        """The receive side of Secure RTP (lc3plus_dec_batch_srtp_unprotect), in front of rtp_parse_device on the same datagram list: raw device pointers only -
        the datagrams in ring, the sources ssrc_key (ascending as uint32) with ctx [n_ssrc, SRTP_CTX_WORDS], state_in / state_out [n_ssrc, SRTP_STATE_WORDS]
        (they may be one array), a workspace of srtp_workspace_bytes(n_items, n_ssrc) bytes -> the accepted datagrams decrypted in place, sizes_out [n_items]
        (rtp_parse_device's dg_sizes), the advanced state and the optional status (uint8), index (int64) [n_items] and stats [SRTP_STATS_WORDS].  Stateless:
        nothing of the batch's streams is read or written.  Queued on hip_stream; returns at once unless sync."""
        _device_call("lc3plus_dec_batch_srtp_unprotect", locals())

    def srtp_unprotect(self, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len=10, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
        """Host convenience: the arrays of plan_srtp_unprotect uploaded, run on the device and downloaded -> the dict plan_srtp_unprotect gives.  Device memory
        through the HIP runtime as in probe(), the workspace too, freed before it returns."""
        return self._srtp_unprotect("srtp", ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, tag_len, optional, ring_capacity)

    def srtp_gcm_unprotect_device(self, n_items, d_ring_ptr, ring_capacity, d_dg_offsets_ptr, d_dg_sizes_ptr, n_ssrc, d_ssrc_key_ptr, d_ctx_ptr, d_state_in_ptr,
                                  d_state_out_ptr, d_sizes_out_ptr, d_workspace_ptr, workspace_bytes, d_status_ptr=None, d_index_ptr=None, d_stats_ptr=None,
                                  hip_stream=None, sync=False):
        """srtp_unprotect_device for the AEAD suites (lc3plus_dec_batch_srtp_gcm_unprotect): the same arguments without tag_len, ctx [n_ssrc,
        SRTP_GCM_CTX_WORDS], sources of 16- and 32-byte keys side by side; the workspace is srtp_workspace_bytes(n_items, n_ssrc) bytes."""
        _device_call("lc3plus_dec_batch_srtp_gcm_unprotect", locals())

    def srtp_gcm_unprotect(self, ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, optional=SRTP_UNPROTECT_OPTIONAL, ring_capacity=None):
        """Host convenience: the arrays of plan_srtp_gcm_unprotect uploaded, run on the device and downloaded -> the dict plan_srtp_gcm_unprotect gives."""
        return self._srtp_unprotect("srtp_gcm", ring, dg_offsets, dg_sizes, ssrc_key, ctx, state, None, optional, ring_capacity)


# what api.py re-exports as its own names: all of the above but the binding's own tools
__all__ = [name for name in dir() if not name.startswith("_") and name not in ("C", "contextlib", "np", "declare", "PARAMS")]
