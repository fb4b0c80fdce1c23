"""The whole wire path on the GPU, call after call (include/lc3plus_batch.h:994-995), held to the host composition of tests/wire_path.py, which
tests/test_wire_path_cpu.py holds to the rule, the oracle's frames and its census:

  sender    set_frame_counts + encode_device_packed (bitrates from device memory) -> egress (in place) -> red_pack -> stamp -> fec_encode -> stamp (FEC list)
            -> protect (media), protect (FEC): queued on one HIP stream with sync = 0, then one wait
  network   on the host: out_offset, out_size and the two destinations downloaded, the receiver's ring and datagram list built by the scenario's network
  receiver  unprotect (both kinds, one table) -> parse (media) + parse (FEC) -> rtcp_stats -> fec_recover -> parse (recovered) -> red_unpack -> probe -> ingest
            -> set_frame_counts + decode_device_packed: queued on one stream, then one wait

Every output array of every step of every call equals the host plan's, with guard elements behind each; the wire, FEC wire, destination and ring buffers are
compared whole; the probe's records equal the oracle's verdict on every unpacked item (frame_probe_ref); PCM and status equal the oracle decoder's.  All state
stays on the device: the next_* / state_out / tail / accumulator arrays of one call are the inputs of the next (two buffers alternating where an output may not
be its input), are only ever compared with the host's, never uploaded, and every call leaves the arrays it read as they were.  Each
library's workspace is allocated once per side at the size of the largest call, filled with 0xA5 before the first call only and guarded behind its end, so a
smaller call sees what a larger one left.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import numpy as np
import pytest

import wire_path as wp
from lc3_harness import sibling_launches
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
GUARD = 16                                             # elements behind every output array
POISON = 0xA5
WORK_GUARD = 64                                        # bytes behind every workspace
SENTINEL = {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A, np.int16: 0x5A5A}
CASES = [("mixed", s) for s in wp.SUITES] + [("realtime", ("srtp", 10)), ("realtime", ("gcm", 16))]
IDS = ["%s-%s%d" % (n, s[0], s[1]) for n, s in CASES]
# one kernel of every sibling library that the sequence must have launched (the Secure RTP suite's by the case)
SIBLINGS = [("egress", "lc3_egress_scatter_kernel"), ("red", "lc3_red_copy_kernel"), ("red", "lc3_red_tail_kernel"), ("red", "lc3_red_unpack_kernel"),
            ("rtp", "lc3_rtp_stamp_kernel"), ("rtp", "lc3_rtp_parse_kernel"), ("fec", "lc3_fec_enc_xor_kernel"), ("fec", "lc3_fec_rec_bytes_kernel"),
            ("rtcp", "lc3_rtcp_walk_kernel"), ("probe", "lc3_probe_full_kernel_g"), ("ingest", "lc3_ingest_item_kernel")]
SUITE_SIBLINGS = {"srtp": [("srtp", "lc3_srtp_protect_kernel"), ("srtp", "lc3_srtp_auth_kernel")], "gcm": [("gcm", "lc3_gcm_protect_kernel"), ("gcm", "lc3_gcm_auth_kernel")]}


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def host():
    made = {}

    def get(name, suite):
        if (name, suite) not in made:
            made[(name, suite)] = wp.run_host(name, suite)
        return made[(name, suite)]
    return get


class _Outs:
    """the output arrays of one call: each starts as its type's sentinel with GUARD elements behind it"""

    def __init__(self, dev):
        self.dev, self.reg = dev, {}

    def new(self, key, shape, dt, extra=0):
        """-> the device pointer of an array of `shape` (and `extra` more elements that belong to it, for a second call's part)"""
        n = int(np.prod(shape)) + extra
        self.reg[key] = (self.dev.put(np.full(n + GUARD, SENTINEL[dt], dt)), n, shape, dt)
        return self.reg[key][0]

    def buf(self, key, nbytes, fill):
        """a byte buffer filled with `fill`, GUARD bytes of it behind its end"""
        self.reg[key] = (self.dev.put(np.full(nbytes + GUARD, fill, np.uint8)), nbytes, (nbytes,), fill)
        return self.reg[key][0]

    def get(self, key, where, written=None, part=None):
        """the array back, the guard behind it intact; written: the entries at and behind it must still hold the sentinel and are given as 0, as the binding's
        plans leave them; part: (first element, shape) of a part of the array"""
        ptr, n, shape, dt = self.reg[key]
        if not isinstance(dt, type):                                  # a byte buffer
            a = self.dev.get(ptr, (n + GUARD,), np.uint8)
            assert (a[n:] == dt).all(), (where, key, "a byte behind the buffer was written")
            return a[:n]
        a = self.dev.get(ptr, (n + GUARD,), dt)
        assert (a[n:] == SENTINEL[dt]).all(), (where, key, "an element behind the output was written")
        a = a[:n]
        if part is not None:
            a, shape = a[part[0]:part[0] + int(np.prod(part[1]))], part[1]
        a = a.reshape(shape)
        if written is not None:
            assert (a[written:] == SENTINEL[dt]).all(), (where, key, "an entry behind the list's length was written")
            a[written:] = 0
        return a


def _same(got, want, where):
    """every array of got equals want's: the call, the step, the array and the first differing index otherwise"""
    for k, g in got.items():
        w = want[k]
        if np.isscalar(w):
            assert int(g) == int(w), (where, k, int(g), int(w))
            continue
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (where, k, "first differing index", bad[0].tolist(), "device", g[tuple(bad[0])], "host", w[tuple(bad[0])], "differing", len(bad))


def _tails(bytes_, sizes):
    """a tail's bytes where its sizes say there are any (the rest of a slot means nothing)"""
    out = np.zeros_like(bytes_)
    for s in range(bytes_.shape[0]):
        for g in range(bytes_.shape[1]):
            k = int(sizes[s, g]) if 0 < sizes[s, g] <= bytes_.shape[2] else 0
            out[s, g, :k] = bytes_[s, g, :k]
    return out


class _State:
    """The state both sides keep in device memory from call to call: name -> two guarded arrays that alternate (`cur` is this call's input, `nxt` its output), or
    one where the call may write its input's array."""

    def __init__(self, dev, start, in_place=("unprotect", "rtcp")):
        self.dev, self.at, self.a = dev, 0, {}
        for k, v in start.items():
            v = np.ascontiguousarray(v)
            dt = v.dtype.type
            two = [dev.put(np.concatenate([v.ravel(), np.full(GUARD, SENTINEL[dt], dt)])), dev.put(np.full(v.size + GUARD, SENTINEL[dt], dt))]
            self.a[k] = (two[:1] * 2 if k in in_place else two, v.shape, dt)

    def cur(self, k):
        return self.a[k][0][self.at]

    def nxt(self, k):
        return self.a[k][0][self.at ^ 1]

    def get(self, k, where, nxt=True):
        ptrs, shape, dt = self.a[k]
        n = int(np.prod(shape))
        a = self.dev.get(ptrs[self.at ^ 1 if nxt else self.at], (n + GUARD,), dt)
        assert (a[n:] == SENTINEL[dt]).all(), (where, k, "an element behind the state was written")
        return a[:n].reshape(shape)

    def flip(self):
        self.at ^= 1


@pytest.mark.parametrize("name,suite", CASES, ids=IDS)
def test_the_whole_wire_path(dev, host, name, suite):
    api = _amd().api
    want = host(name, suite)
    sc, cap = want["scenario"], wp.wire_bytes(want["scenario"])
    S, N, CH, MAXB = wp.S, wp.N, wp.CH, wp.MAXB
    Tmax = max(sc["T"])
    infix = "srtp" if suite[0] == "srtp" else "srtp_gcm"
    tag = [suite[1]] if suite[0] == "srtp" else []
    _, _, _, ctx, fctx = wp.contexts(suite)
    keys, kind, route = wp.source_table()
    siblings = SIBLINGS + SUITE_SIBLINGS[suite[0]]
    before = {k: sibling_launches(*k) for k in siblings}
    enc = _amd().Batch(S, wp.FS, CH, wp.MS, wp.HR, [64000] * S, device=0)
    dec = _amd().DecBatch(S, wp.FS, CH, wp.MS, wp.HR, None, device=0)
    u32 = wp._u32
    # what never changes: the tables of both sides
    c_ssrc, c_fssrc, c_red_pt, c_blk_pt, c_fec_pt = dev.put(u32(wp.SSRC)), dev.put(u32(wp.FEC_SSRC)), dev.put(np.full(S, wp.RED_PT, np.int32)), \
        dev.put(np.full(S, wp.BLOCK_PT, np.int32)), dev.put(np.full(S, wp.FEC_PT, np.int32))
    c_ctx, c_fctx = dev.put(ctx), dev.put(fctx)
    c_keys, c_ctx12 = dev.put(u32(keys)), dev.put(np.ascontiguousarray(np.where(kind[:, None] == 0, ctx[route], fctx[route])))
    mkey, mstream = api.rtp_sort_ssrc(wp.SSRC, np.arange(S))
    fkey, fstream = api.rtp_sort_ssrc(wp.FEC_SSRC, np.arange(S))
    c_mkey, c_mstream, c_fkey, c_fstream = dev.put(mkey), dev.put(mstream), dev.put(fkey), dev.put(fstream)
    # the state, on the device from here on
    st = _State(dev, want["start"])
    # one workspace per library and side, sized for the largest call, poisoned once
    sizes = dict(egress=api.egress_work_bytes(S, Tmax), red=api.red_work_bytes(S * Tmax), fec=api.fec_work_bytes(S, Tmax), unprotect=api.srtp_workspace_bytes(cap["max_dg"], 2 * S),
                 rtcp=api.rtcp_workspace_bytes(cap["max_dg"], S), recover=api.fec_recover_work_bytes(S, wp.WINDOW))
    assert all(v > 0 for v in sizes.values()), sizes
    work = {k: dev.put(np.full(v + WORK_GUARD, POISON, np.uint8)) for k, v in sizes.items()}
    s1 = dev.stream()
    sent = []
    for c, T in enumerate(sc["T"]):
        h, n, Q = want["calls"][c], S * T, cap["max_fec"]
        inp = h["inputs"]
        total = inp["frames"].size - 8
        o = _Outs(dev)
        # ---- the sender ----
        d_pcm, d_br, d_cnt = dev.put(inp["pcm"]), dev.put(inp["bitrates"]), dev.put(inp["counts"])
        d_depth, d_group, d_flush = dev.put(h["depth"]), dev.put(h["group"]), dev.put(np.full(S, h["flush"], np.uint8))
        d_out = o.buf("frames", total + 8, 0xC3)
        d_off, d_tot, d_nb, d_fl = o.new("enc_offsets", (S, T), np.int64), o.new("enc_total", (1,), np.int64), o.new("enc_num_bytes", (S, T), np.int32), o.new("enc_flags", (S, T), np.uint8)
        e = {k: o.new("e_" + k, (n,), dt) for k, dt in (("pkt_route", np.int32), ("pkt_seq", np.int32), ("pkt_frame", np.int32), ("pkt_offset", np.int64), ("pkt_size", np.int32),
                                                       ("pkt_flags", np.uint8))}
        e_np, e_wt, e_stats, e_cs = o.new("e_n_packets", (1,), np.int64), o.new("e_wire_total", (1,), np.int64), o.new("e_stats", (S, 4), np.int32), o.new("e_cell_status", (S, T), np.uint8)
        d_wire = o.buf("wire", cap["wire"], wp.FILL)
        r_off, r_size, r_flags, r_blocks = o.new("r_red_offset", (n,), np.int64), o.new("r_red_size", (n,), np.int32), o.new("r_red_flags", (n,), np.uint8), o.new("r_red_blocks", (n,), np.uint8)
        r_wt, r_stats = o.new("r_wire_total", (1,), np.int64), o.new("r_route_stats", (S, 4), np.int32)
        s_pst = o.new("s_pkt_status", (n,), np.uint8)
        d_fwire = o.buf("fec_wire", cap["fec_wire"], wp.FILL)
        f = {k: o.new("f_" + k, (Q,), dt) for k, dt in (("fec_route", np.int32), ("fec_seq", np.int32), ("fec_frame", np.int32), ("fec_offset", np.int64), ("fec_size", np.int32),
                                                       ("fec_flags", np.uint8), ("fec_mask", np.int32))}
        f_n, f_stats, fs_pst = o.new("f_n_fec", (1,), np.int64), o.new("f_route_stats", (S, 4), np.int32), o.new("fs_pkt_status", (Q,), np.uint8)
        d_dst, d_fdst = o.buf("dst", cap["dst"], wp.FILL), o.buf("fec_dst", cap["fec_dst"], wp.FILL)
        p_off, p_size, p_st = o.new("p_out_offset", (n,), np.int64), o.new("p_out_size", (n,), np.int32), o.new("p_out_status", (n,), np.uint8)
        fp_off, fp_size, fp_st = o.new("fp_out_offset", (Q,), np.int64), o.new("fp_out_size", (Q,), np.int32), o.new("fp_out_status", (Q,), np.uint8)
        dev.sync()
        enc.set_frame_counts(d_cnt)
        enc.encode_device_packed(d_pcm, 16, T, d_out, total, api.PACK_STREAM_MAJOR, d_br, None, d_off, d_tot, d_nb, d_fl, s1, sync=False)
        enc.egress_device(T, d_out, total, d_off, d_nb, MAXB, S, st.cur("seq_base"), e["pkt_route"], e["pkt_seq"], e["pkt_frame"], e["pkt_offset"], e["pkt_size"], e_np, work["egress"],
                          None, 0, d_cnt, None, 16, api.PACK_STREAM_MAJOR, None, 0, 0, 1, e["pkt_flags"], e_wt, st.nxt("seq_base"), e_stats, e_cs, s1, sync=False)
        enc.red_pack_device(T, d_out, total, d_off, d_nb, MAXB, S, n, e_np, e["pkt_route"], e["pkt_frame"], wp.MAX_DEPTH, c_blk_pt, N, 1 << 20, d_wire, cap["wire"], r_off, r_size,
                            work["red"], wp.ROOM, wp.ALIGN, None, 0, d_cnt, None, d_depth, st.cur("tail_bytes"), st.cur("tail_sizes"), api.red_tail_stride(MAXB),
                            st.nxt("tail_bytes"), st.nxt("tail_sizes"), r_flags, r_blocks, r_wt, r_stats, s1, sync=False)
        enc.rtp_stamp_device(n, e_np, e["pkt_route"], e["pkt_seq"], e["pkt_frame"], r_off, r_size, S, T, c_ssrc, st.cur("ts_base"), c_red_pt, N, d_wire, cap["wire"], wp.ROOM, 0,
                             r_flags, api.RTP_MARKER_AFTER_HOLE, e_cs, st.cur("resume"), e_stats, s_pst, st.nxt("ts_base"), st.nxt("resume"), s1, sync=False)
        enc.fec_encode_device(n, e_np, e["pkt_route"], e["pkt_frame"], r_off, r_size, d_wire, cap["wire"], S, T, st.cur("seq_base"), d_group, st.cur("fec_seq_base"), d_fwire,
                              cap["fec_wire"], wp.FEC_STRIDE, Q, f_n, f["fec_route"], f["fec_seq"], f["fec_frame"], f["fec_offset"], f["fec_size"], work["fec"], wp.ROOM, 0,
                              wp.FEC_ROOM, s_pst, e_stats, d_flush, st.cur("fec_state"), st.cur("fec_acc"), st.nxt("fec_state"), st.nxt("fec_acc"), wp.ACC_STRIDE, f["fec_flags"],
                              f["fec_mask"], st.nxt("fec_seq_base"), f_stats, s1, sync=False)
        enc.rtp_stamp_device(Q, f_n, f["fec_route"], f["fec_seq"], f["fec_frame"], f["fec_offset"], f["fec_size"], S, T, c_fssrc, st.cur("ts_base"), c_fec_pt, N, d_fwire,
                             cap["fec_wire"], wp.FEC_ROOM, 0, f["fec_flags"], api.RTP_MARKER_NEVER, None, None, None, fs_pst, None, None, s1, sync=False)
        getattr(enc, infix + "_protect_device")(n, e_np, e["pkt_route"], r_off, r_size, s_pst, d_wire, cap["wire"], S, c_ctx, st.cur("roc"), st.cur("seq_base"), d_dst, cap["dst"],
                                                wp.DST_STRIDE, p_off, p_size, p_st, *tag, wp.ROOM, 0, st.nxt("seq_base"), st.nxt("roc"), s1, sync=False)
        getattr(enc, infix + "_protect_device")(Q, f_n, f["fec_route"], f["fec_offset"], f["fec_size"], fs_pst, d_fwire, cap["fec_wire"], S, c_fctx, st.cur("fec_roc"),
                                                st.cur("fec_seq_base"), d_fdst, cap["fec_dst"], wp.DST_STRIDE, fp_off, fp_size, fp_st, *tag, wp.FEC_ROOM, 0,
                                                st.nxt("fec_seq_base"), st.nxt("fec_roc"), s1, sync=False)
        dev.stream_sync(s1)
        w = lambda step: (name, suite, "call", c, "step", step)
        got_frames = o.get("frames", w("encode"))
        there = np.arange(T)[None, :] < inp["counts"][:, None]          # an absent frame's offset is read by nobody
        _same(dict(offsets=np.where(there, o.get("enc_offsets", w("encode")), 0), num_bytes=o.get("enc_num_bytes", w("encode")), flags=o.get("enc_flags", w("encode")),
                   frames=got_frames[:total]),
              dict(offsets=np.where(there, inp["offsets"], 0), num_bytes=inp["num_bytes"], flags=np.where(there, 0, api.ENC_FL_ABSENT).astype(np.uint8),
                   frames=inp["frames"][:total]), w("encode"))
        assert int(o.get("enc_total", w("encode"))[0]) == total and (got_frames[total:] == 0xC3).all(), w("encode")
        npk = int(o.get("e_n_packets", w("egress"))[0])
        ge = {k: o.get("e_" + k, w("egress"), written=npk) for k in e}
        ge.update(n_packets=npk, wire_total=int(o.get("e_wire_total", w("egress"))[0]), next_seq=st.get("seq_base", w("egress")), stats=o.get("e_stats", w("egress")),
                  cell_status=o.get("e_cell_status", w("egress")))
        _same(ge, h["egress"], w("egress"))
        gr = dict(red_offset=o.get("r_red_offset", w("red_pack"), npk), red_size=o.get("r_red_size", w("red_pack"), npk), red_flags=o.get("r_red_flags", w("red_pack"), npk),
                  red_blocks=o.get("r_red_blocks", w("red_pack"), npk), wire_total=int(o.get("r_wire_total", w("red_pack"))[0]), route_stats=o.get("r_route_stats", w("red_pack")),
                  tail_sizes=st.get("tail_sizes", w("red_pack")))
        gr["tail_bytes"] = _tails(st.get("tail_bytes", w("red_pack")), gr["tail_sizes"])
        _same(gr, dict(h["red"], tail_bytes=_tails(h["red"]["tail_bytes"], h["red"]["tail_sizes"])), w("red_pack"))
        _same(dict(pkt_status=o.get("s_pkt_status", w("stamp"), npk), next_ts=st.get("ts_base", w("stamp")), next_resume=st.get("resume", w("stamp")), wire=o.get("wire", w("stamp"))),
              h["stamp"], w("stamp"))
        nf = int(o.get("f_n_fec", w("fec_encode"))[0])
        gf = {k: o.get("f_" + k, w("fec_encode"), written=min(nf, Q)) for k in f}
        gf.update(n_fec=nf, state=st.get("fec_state", w("fec_encode")), acc=st.get("fec_acc", w("fec_encode")), next_fec_seq=st.get("fec_seq_base", w("fec_encode")),
                  route_stats=o.get("f_route_stats", w("fec_encode")))
        _same(gf, h["fec"], w("fec_encode"))
        _same(dict(pkt_status=o.get("fs_pkt_status", w("stamp (FEC)"), min(nf, Q)), wire=o.get("fec_wire", w("stamp (FEC)"))), h["fec_stamp"], w("stamp (FEC)"))
        gp = dict(out_offset=o.get("p_out_offset", w("protect"), npk), out_size=o.get("p_out_size", w("protect"), npk), out_status=o.get("p_out_status", w("protect"), npk),
                  next_roc=st.get("roc", w("protect")), dst=o.get("dst", w("protect")))
        _same(gp, h["protect"], w("protect"))
        gfp = dict(out_offset=o.get("fp_out_offset", w("protect (FEC)"), min(nf, Q)), out_size=o.get("fp_out_size", w("protect (FEC)"), min(nf, Q)),
                   out_status=o.get("fp_out_status", w("protect (FEC)"), min(nf, Q)), next_roc=st.get("fec_roc", w("protect (FEC)")), dst=o.get("fec_dst", w("protect (FEC)")))
        _same(gfp, h["fec_protect"], w("protect (FEC)"))
        # ---- the network, on the host, from what the device sent ----
        sent.append(dict(egress=ge, fec=gf, protect=gp, fec_protect=gfp))
        net = wp.network_call(sc, c, sent)
        assert net["items"] == h["net"]["items"]
        _same({k: net[k] for k in ("ring", "dg_offsets", "dg_sizes", "arrival")}, h["net"], w("network"))
        # ---- the receiver ----
        m = len(net["dg_offsets"])
        d_ring = dev.put(np.concatenate([net["ring"], np.full(GUARD, wp.FILL, np.uint8)]))
        o.reg["ring"] = (d_ring, cap["ring"], (cap["ring"],), wp.FILL)
        d_dgo, d_dgs, d_arr = dev.put(net["dg_offsets"]), dev.put(net["dg_sizes"]), dev.put(net["arrival"])
        u_sizes, u_st, u_idx, u_stats = o.new("u_sizes", (m,), np.int32), o.new("u_status", (m,), np.uint8), o.new("u_index", (m,), np.int64), o.new("u_stats", (16,), np.int32)
        items = ("stream", np.int32), ("seq", np.int32), ("offsets", np.int64), ("num_bytes", np.int32), ("timestamp", np.int32)
        i_ = {k: o.new("i_" + k, (m,), dt, extra=m) for k, dt in items}                      # the media items, and behind them the recovered packets' items
        g_ = {k: o.new("g_" + k, (m,), dt) for k, dt in items}
        for who in ("i", "g", "x"):
            o.new(who + "_marker", (m,), np.uint8), o.new(who + "_status", (m,), np.uint8), o.new(who + "_stats", (16,), np.int32)
        rr_blocks, rr_ext, rr_ist, rr_ss = o.new("rr_blocks", (S, api.RR_BLOCK_BYTES), np.uint8), o.new("rr_ext_seq", (m,), np.int32), o.new("rr_item_status", (m,), np.uint8), \
            o.new("rr_stream_stats", (S, 4), np.int32)
        v_off, v_size, v_seq, v_st, v_stats = o.new("v_rec_dg_offsets", (m,), np.int64), o.new("v_rec_dg_sizes", (m,), np.int32), o.new("v_rec_seq", (m,), np.int32), \
            o.new("v_status", (m,), np.uint8), o.new("v_stats", (16,), np.int32)
        K = 2 * m * (wp.MAX_DEPTH + 1)
        k_ = {k: o.new("k_" + k, (K,), dt) for k, dt in items + (("gen", np.uint8),)}
        k_st, k_stats = o.new("k_status", (2 * m,), np.uint8), o.new("k_stats", (16,), np.int32)
        d_info = o.new("probe_info", (K, CH, api.FRAME_INFO_WORDS), np.int32)
        n_oo, n_onb, n_ci, n_cnt, n_stats, n_ist = o.new("n_offsets", (S, T), np.int64), o.new("n_num_bytes", (S, T), np.int32), o.new("n_cell_item", (S, T), np.int32), \
            o.new("n_counts", (S,), np.int32), o.new("n_stats", (S, 4), np.int32), o.new("n_item_status", (K,), np.uint8)
        d_pcm_out, d_dst_st = o.new("pcm", (S, T, CH, N), np.int16), o.new("dec_status", (S, T), np.uint8)
        second = lambda key, size: i_[key] + size * m
        dev.sync()
        getattr(dec, infix + "_unprotect_device")(m, d_ring, cap["ring"], d_dgo, d_dgs, 2 * S, c_keys, c_ctx12, st.cur("unprotect"), st.nxt("unprotect"), u_sizes, work["unprotect"],
                                                  sizes["unprotect"], *tag, u_st, u_idx, u_stats, s1, sync=False)
        dec.rtp_parse_device(m, d_ring, cap["ring"], d_dgo, u_sizes, S, c_mkey, c_mstream, i_["stream"], i_["seq"], i_["offsets"], i_["num_bytes"], c_red_pt, 0, i_["timestamp"],
                             o.reg["i_marker"][0], o.reg["i_status"][0], o.reg["i_stats"][0], s1, sync=False)
        dec.rtp_parse_device(m, d_ring, cap["ring"], d_dgo, u_sizes, S, c_fkey, c_fstream, g_["stream"], g_["seq"], g_["offsets"], g_["num_bytes"], c_fec_pt, 0, g_["timestamp"],
                             o.reg["g_marker"][0], o.reg["g_status"][0], o.reg["g_stats"][0], s1, sync=False)
        dec.rtcp_stats_device(m, i_["stream"], i_["seq"], i_["timestamp"], d_arr, S, st.cur("rtcp"), st.nxt("rtcp"), work["rtcp"], sizes["rtcp"], 1, c_ssrc, None, None, rr_blocks,
                              rr_ext, rr_ist, rr_ss, s1, sync=False)
        dec.fec_recover_device(m, d_ring, cap["ring"], d_dgo, u_sizes, i_["stream"], i_["seq"], m, g_["stream"], g_["offsets"], g_["num_bytes"], wp.WINDOW, c_ssrc, cap["rec_offset"],
                               wp.REC_STRIDE, v_off, v_size, v_seq, work["recover"], v_st, v_stats, s1, sync=False)
        dec.rtp_parse_device(m, d_ring, cap["ring"], v_off, v_size, S, c_mkey, c_mstream, second("stream", 4), second("seq", 4), second("offsets", 8), second("num_bytes", 4), c_red_pt,
                             0, second("timestamp", 4), o.reg["x_marker"][0], o.reg["x_status"][0], o.reg["x_stats"][0], s1, sync=False)
        dec.red_unpack_device(2 * m, i_["stream"], i_["seq"], i_["offsets"], i_["num_bytes"], d_ring, cap["ring"], wp.MAX_DEPTH, N, k_["stream"], k_["seq"], k_["offsets"],
                              k_["num_bytes"], i_["timestamp"], c_blk_pt, k_["timestamp"], k_["gen"], k_st, k_stats, s1, sync=False)
        dec.probe_device(d_ring, cap["ring"], k_["offsets"], k_["num_bytes"], MAXB, K, d_info, api.PROBE_FULL, s1, sync=False)
        dec.ingest_device(K, k_["stream"], k_["seq"], k_["offsets"], k_["num_bytes"], st.cur("base"), T, n_oo, n_onb, n_ci, n_cnt, 16, d_info, None, st.nxt("base"), n_stats, n_ist,
                          s1, sync=False)
        dec.set_frame_counts(n_cnt)
        dec.decode_device_packed(d_ring, cap["ring"], n_oo, T, d_pcm_out, n_onb, MAXB, None, d_dst_st, 16, s1, sync=False)
        dev.stream_sync(s1)
        _same(dict(state=st.get("unprotect", w("unprotect")), sizes=o.get("u_sizes", w("unprotect")), status=o.get("u_status", w("unprotect")), index=o.get("u_index", w("unprotect")),
                   stats=o.get("u_stats", w("unprotect"))), h["unprotect"], w("unprotect"))
        for who, step, part in (("i", "parse", (0, (m,))), ("g", "fec_parse", None), ("i", "rec_parse", (m, (m,)))):
            x = "x" if step == "rec_parse" else who
            got = {k: o.get(who + "_" + k, w(step), part=part) for k, _ in items}
            got.update(marker=o.get(x + "_marker", w(step)), status=o.get(x + "_status", w(step)), stats=o.get(x + "_stats", w(step)))
            _same(got, h[step], w(step))
        _same(dict(state=st.get("rtcp", w("rtcp_stats")), blocks=o.get("rr_blocks", w("rtcp_stats")), ext_seq=o.get("rr_ext_seq", w("rtcp_stats")),
                   item_status=o.get("rr_item_status", w("rtcp_stats")), stream_stats=o.get("rr_stream_stats", w("rtcp_stats"))), h["rtcp"], w("rtcp_stats"))
        ring = o.get("ring", w("fec_recover"))
        _same(dict(ring=ring, rec_dg_offsets=o.get("v_rec_dg_offsets", w("fec_recover")), rec_dg_sizes=o.get("v_rec_dg_sizes", w("fec_recover")),
                   rec_seq=o.get("v_rec_seq", w("fec_recover")), status=o.get("v_status", w("fec_recover")), stats=o.get("v_stats", w("fec_recover"))), h["recover"], w("fec_recover"))
        got = {k: o.get("k_" + k, w("red_unpack")) for k, _ in items + (("gen", None),)}
        got.update(status=o.get("k_status", w("red_unpack")), stats=o.get("k_stats", w("red_unpack")))
        _same(got, h["unpack"], w("red_unpack"))
        _same(dict(info=o.get("probe_info", w("probe"))), h["probe"], w("probe"))
        gi = dict(offsets=o.get("n_offsets", w("ingest")), num_bytes=o.get("n_num_bytes", w("ingest")), cell_item=o.get("n_cell_item", w("ingest")), counts=o.get("n_counts", w("ingest")),
                  next_base=st.get("base", w("ingest")), stats=o.get("n_stats", w("ingest")), item_status=o.get("n_item_status", w("ingest")))
        _same(gi, h["ingest"], w("ingest"))
        pcm, dst = o.get("pcm", w("decode")), o.get("dec_status", w("decode"))
        for s in range(S):
            k = int(gi["counts"][s])
            _same(dict(pcm=pcm[s, :k], status=dst[s, :k]), dict(pcm=want["pcm"][c][s, :k], status=want["status"][c][s, :k]), w("decode") + ("stream", s))
            assert (pcm[s, k:] == SENTINEL[np.int16]).all(), (w("decode"), s, "a frame behind the stream's count was written")
        # no call wrote the state it read (the two that may, unprotect and rtcp_stats, were given one array for both)
        was = {k: st.get(k, w("inputs"), nxt=False) for k in h["state_in"] if k not in ("unprotect", "rtcp")}
        was["tail_bytes"] = _tails(was["tail_bytes"], was["tail_sizes"])
        _same(was, dict(h["state_in"], tail_bytes=_tails(h["state_in"]["tail_bytes"], h["state_in"]["tail_sizes"])), w("inputs"))
        st.flip()
    enc.set_frame_counts(None)
    dec.set_frame_counts(None)
    for k, v in sizes.items():
        assert (dev.get(work[k] + v, (WORK_GUARD,), np.uint8) == POISON).all(), ("a byte behind the workspace was written", k)
    for k in siblings:
        assert sibling_launches(*k) > before[k], ("the sequence never launched", k)
    enc.close()
    dec.close()
