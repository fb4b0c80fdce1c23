"""What test_gpu_srtp.py and test_gpu_gcm.py share: guarded device arrays, the comparison of a result dict with a plan's, an unprotect and a protect call of
either suite on the device with guard bytes around everything, and the sender-to-receiver chain.  A suite is named by the infix of its methods ("srtp",
"srtp_gcm") and by tag_len: the HMAC calls' argument, None for the AEAD calls, which take none and append SRTP_GCM_TAG_BYTES.  Device buffers through ctypes
(test_gpu_dec_varsize_device._Hip)."""
import numpy as np
import pytest

import hostile_frames as hf
from test_gpu_dec_varsize_device import _Hip

GUARD = 16                                             # elements behind every output array
SENTINEL = {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A}


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _dec(S=1):
    return _amd().DecBatch(S, 48000, 1, 10.0, 0, None, device=0)


def _guarded(dev, n, dt):
    return dev.put(np.full(n + GUARD, SENTINEL[dt], dt))


def _ungard(dev, ptr, n, dt, name):
    got = dev.get(ptr, (n + GUARD,), dt)
    assert (got[n:] == SENTINEL[dt]).all(), ("an element behind the output was written", name)
    return got[:n]


def _u32(a):
    return (np.asarray(a).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _same(got, want, name):
    for k in want:
        if want[k] is None:
            assert got[k] is None, (name, k)
            continue
        bad = np.argwhere(np.asarray(got[k]).reshape(-1) != np.asarray(want[k]).reshape(-1))
        assert got[k].shape == want[k].shape and len(bad) == 0, (name, k, "first differing elements", bad[:6].ravel().tolist())


def _tag(tag_len):
    """tag_len as the calls of a suite take it between their positional arguments"""
    return [] if tag_len is None else [tag_len]


def unprotect(dev, bat, infix, tag_len, c, optional=("status", "index", "stats"), in_place=False, ring_shift=0, hip_stream=None):
    """the case on the device -> the dict the suite's unprotect plan gives.  The ring lies ring_shift bytes behind an aligned address; with in_place state_out is
    state_in"""
    api = _amd().api
    n, S = len(c["offs"]), len(c["ssrc_key"])
    ring = np.concatenate([np.full(ring_shift, 0x77, np.uint8), c["ring"]])
    d_ring = dev.put(ring)
    d_state_in = dev.put(np.ascontiguousarray(c["state"]))
    d_state_out = d_state_in if in_place else _guarded(dev, S * 8, np.int32)
    wb = api.srtp_workspace_bytes(n, S)
    d_work = dev.put(np.full(wb + 64, 0x3C, np.uint8))
    d_sizes = _guarded(dev, n, np.int32)
    d_status = _guarded(dev, n, np.uint8) if "status" in optional else None
    d_index = _guarded(dev, n, np.int64) if "index" in optional else None
    d_stats = _guarded(dev, 16, np.int32) if "stats" in optional else None
    getattr(bat, infix + "_unprotect_device")(n, d_ring + ring_shift, c["ring"].size, dev.put(c["offs"]), dev.put(c["sizes"]), S, dev.put(c["ssrc_key"]),
                                              dev.put(c["ctx"]), d_state_in, d_state_out, d_sizes, d_work + 1, wb, *_tag(tag_len), d_status, d_index, d_stats, hip_stream,
                                              sync=True)
    whole = dev.get(d_ring, (ring.size,), np.uint8)
    assert (whole[:ring_shift] == 0x77).all()
    assert (dev.get(d_work, (wb + 64,), np.uint8)[wb + 1:] == 0x3C).all(), "the workspace was written past its size"
    state = dev.get(d_state_in, (S, 8), np.int32) if in_place else _ungard(dev, d_state_out, S * 8, np.int32, "state").reshape(S, 8)
    if not in_place:
        assert np.array_equal(dev.get(d_state_in, (S, 8), np.int32), c["state"])
    return dict(ring=whole[ring_shift:], state=state, sizes=_ungard(dev, d_sizes, n, np.int32, "sizes"),
                status=_ungard(dev, d_status, n, np.uint8, "status") if d_status else None, index=_ungard(dev, d_index, n, np.int64, "index") if d_index else None,
                stats=_ungard(dev, d_stats, 16, np.int32, "stats") if d_stats else None)


def protect(dev, bat, infix, tag_len, c, guard, dst_shift, with_next=True, hip_stream=None):
    """the protect list on the device -> the dict the suite's protect plan gives; guard: the bytes in front of and behind the destination (the case module's)"""
    m = c["max_packets"]
    cap = c["dst_capacity"]
    dst0 = np.full(guard + dst_shift + cap + guard, 0x6B, np.uint8)
    d_dst = dev.put(dst0)
    d_oo, d_os, d_ost = _guarded(dev, m, np.int64), _guarded(dev, m, np.int32), _guarded(dev, m, np.uint8)
    d_next = _guarded(dev, 2, np.int32) if with_next else None
    getattr(bat, infix + "_protect_device")(m, dev.put(np.array([c["n_packets"]], np.int64)), dev.put(c["route"]), dev.put(c["off"]), dev.put(c["size"]),
                                            dev.put(c["status"]), dev.put(c["wire"]), c["wire"].size, 2, dev.put(c["ctx"]), dev.put(c["roc"]), dev.put(c["seq_base"]),
                                            d_dst + guard + dst_shift, cap, c["stride"], d_oo, d_os, d_ost, *_tag(tag_len), c["hr"], c["pr"],
                                            dev.put(c["next_seq"]) if with_next else None, d_next, hip_stream, sync=True)
    whole = dev.get(d_dst, (dst0.size,), np.uint8)
    lo = guard + dst_shift
    assert (whole[:lo] == 0x6B).all() and (whole[lo + cap:] == 0x6B).all(), "a byte outside the destination was written"
    return dict(dst=whole[lo:lo + cap], out_offset=_ungard(dev, d_oo, m, np.int64, "out_offset"), out_size=_ungard(dev, d_os, m, np.int32, "out_size"),
                out_status=_ungard(dev, d_ost, m, np.uint8, "out_status"), next_roc=_ungard(dev, d_next, 2, np.int32, "next_roc") if with_next else None)


def sender_to_receiver(dev, infix, tag_len, cases, ref):
    """encode_packed -> egress -> stamp -> protect and unprotect -> parse -> probe -> ingest on the protect call's output, all queued on one HIP stream with
    sync = 0 and one wait at the end.  The protected packets are the host plan's on the stamped wire buffer; every frame the egress sent stands in the ingest's
    tables, byte for byte the oracle encoder's, and the receiver's state has advanced to every route's last sequence number across 65535 -> 0.  cases, ref: the
    suite's case module (keys_for, state_block) and restatement (its status constants).  -> S, the contexts and which routes crossed 65535, for what the
    caller asserts of its suite"""
    from test_gpu_egress import _sender
    api = _amd().api
    plan_protect, plan_unprotect = getattr(api, "plan_%s_protect" % infix), getattr(api, "plan_%s_unprotect" % infix)
    geom = "48k_10_128B"
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    sc = _sender(geom)
    S, T, N, size = sc["S"], sc["T"], sc["N"], sc["size"]
    proom, align = 3, 1
    room = 12 + proom
    present = int(np.clip(sc["counts"], 0, T).sum())
    buf = present * size + 64
    n = S * T
    wire_bytes = n * (room + size + align)
    stride = room + size + (api.SRTP_GCM_TAG_BYTES if tag_len is None else tag_len) + 1
    dst_bytes = n * stride
    enc = _amd().Batch(S, fs, ch, ms, hr, [sc["rate"]] * S, device=0)
    dec = _amd().DecBatch(S, fs, ch, ms, hr, None, device=0)
    i32, i64, u8 = (lambda k, v=-7: dev.put(np.full(k, v, np.int32))), (lambda k, v=-7: dev.put(np.full(k, v, np.int64))), (lambda k, v=0xEE: dev.put(np.full(k, v, np.uint8)))
    d_pcm_in, d_cnt, d_out = dev.put(sc["pcm"]), dev.put(sc["counts"]), u8(buf, 0xC3)
    d_off, d_tot, d_nb, d_fl = i64((S, T)), i64(1), i32((S, T)), u8((S, T))
    seq_base = (65530 + np.arange(S)).astype(np.int32)
    ssrc = 0x7FFFFFF0 + 7 * np.arange(S)
    roc = np.array([0, 1, 2, 0xFFFFFFFE, 4, 5], np.uint32)[:S]
    keys = [cases.keys_for(s) for s in range(S)]
    ctx = np.stack([k.ctx for k in keys]).view(np.int32)
    state = np.array([cases.state_block(1, int(roc[s]), int(seq_base[s]) - 1, 1) if s % 2 else cases.state_block(0, int(roc[s])) for s in range(S)], np.uint32).view(np.int32)
    d_base, d_ssrc, d_tsb, d_pt = dev.put(seq_base), dev.put(_u32(ssrc)), dev.put(_u32(1000 * np.arange(S))), dev.put(np.full(S, 96, np.int32))
    d_sid, d_ctx, d_roc, d_state = dev.put(np.arange(S, dtype=np.int32)), dev.put(ctx), dev.put(roc.view(np.int32)), dev.put(state)
    d_wire, d_dst = u8(wire_bytes, 0xA5), u8(dst_bytes + 8, 0x6B)
    p_route, p_seq, p_frame, p_off, p_size, p_flags = i32(n), i32(n), i32(n), i64(n, -1), i32(n, 0), u8(n)
    d_np, d_wt, d_next, d_stats, d_cs = i64(1), i64(1), i32(S), i32((S, 4)), u8((S, T))
    work = dev.put(np.zeros(api.egress_work_bytes(S, T) // 8 + 1, np.int64))
    d_pst, d_nts = u8(n), i32(S)
    o_off, o_size, o_st, d_nroc = i64(n, -1), i32(n, 0), u8(n), i32(S)     # offset -1 behind n_packets: the unprotect refuses those as RANGE
    wb = api.srtp_workspace_bytes(n, S)
    d_swork = dev.put(np.zeros(wb, np.uint8))
    u_sizes, u_st, u_idx, u_stats = i32(n), u8(n), i64(n), i32(16)
    i_stream, i_seq, i_off, i_nb, i_st = i32(n), i32(n), i64(n), i32(n), u8(n)
    d_info = dev.put(np.zeros((n, ch, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci, d_cnt2, d_nb2 = i64((S, T)), i32((S, T)), i32((S, T)), i32(S), i32(S)
    dev.sync()
    s1 = dev.stream()
    enc.set_frame_counts(d_cnt)
    enc.encode_device_packed(d_pcm_in, 16, T, d_out, buf, api.PACK_FRAME_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, s1, sync=False)
    enc.egress_device(T, d_out, buf, d_off, d_nb, size, S, d_base, p_route, p_seq, p_frame, p_off, p_size, d_np, work, d_fl, api.ENC_FL_PACK_CAP, d_cnt, None, 16,
                      api.PACK_FRAME_MAJOR, d_wire, wire_bytes, room, align, p_flags, d_wt, d_next, d_stats, d_cs, s1, sync=False)
    enc.rtp_stamp_device(n, d_np, p_route, p_seq, p_frame, p_off, p_size, S, T, d_ssrc, d_tsb, d_pt, N, d_wire, wire_bytes, room, proom, p_flags,
                         api.RTP_MARKER_NEVER, None, None, d_stats, d_pst, d_nts, None, s1, sync=False)
    getattr(enc, infix + "_protect_device")(n, d_np, p_route, p_off, p_size, d_pst, d_wire, wire_bytes, S, d_ctx, d_roc, d_base, d_dst + 3, dst_bytes, stride, o_off, o_size,
                                            o_st, *_tag(tag_len), room, proom, d_next, d_nroc, s1, sync=False)
    getattr(dec, infix + "_unprotect_device")(n, d_dst + 3, dst_bytes, o_off, o_size, S, d_ssrc, d_ctx, d_state, d_state, u_sizes, d_swork, wb, *_tag(tag_len), u_st, u_idx,
                                              u_stats, s1, sync=False)
    dec.rtp_parse_device(n, d_dst + 3, dst_bytes, o_off, u_sizes, S, d_ssrc, d_sid, i_stream, i_seq, i_off, i_nb, d_pt, proom, None, None, i_st, None, s1, sync=False)
    dec.probe_device(d_dst + 3, dst_bytes, i_off, i_nb, size, n, d_info, api.PROBE_FULL, s1, sync=False)
    dec.ingest_device(n, i_stream, i_seq, i_off, i_nb, d_base, T, d_oo, d_onb, d_ci, d_cnt2, 16, d_info, None, d_nb2, None, None, s1, sync=False)
    dev.stream_sync(s1)
    enc.set_frame_counts(None)
    k = int(dev.get(d_np, (1,), np.int64)[0])
    assert k == present
    lst = {x: dev.get(p, (n,), dt) for x, p, dt in (("route", p_route, np.int32), ("seq", p_seq, np.int32), ("frame", p_frame, np.int32), ("off", p_off, np.int64),
                                                     ("size", p_size, np.int32))}
    wire, pst = dev.get(d_wire, (wire_bytes,), np.uint8), dev.get(d_pst, (n,), np.uint8)
    next_seq = dev.get(d_next, (S,), np.int32)
    # the protect call against the host plan on the stamped wire buffer; the unprotect call has since decrypted the destination in place, so the plan's
    # destination is held to the unprotect plan's input and the device's to its output
    want = plan_protect(lst["route"], lst["off"], lst["size"], pst, wire, ctx, roc, seq_base, np.full(dst_bytes, 0x6B, np.uint8), stride, *_tag(tag_len), room, proom,
                        next_seq=next_seq, n_packets=k)
    assert (want["out_status"][:k] == ref.PROTECTED).all()
    got_off, got_size = dev.get(o_off, (n,), np.int64), dev.get(o_size, (n,), np.int32)
    assert np.array_equal(got_off[:k], want["out_offset"][:k]) and np.array_equal(got_size[:k], want["out_size"][:k]) and (got_off[k:] == -1).all()
    assert np.array_equal(dev.get(o_st, (n,), np.uint8)[:k], want["out_status"][:k]) and np.array_equal(dev.get(d_nroc, (S,), np.int32), want["next_roc"])
    wrapped = (seq_base.astype(np.int64) & 0xFFFF) + np.clip(sc["counts"], 0, T) > 65535
    assert np.array_equal(want["next_roc"], _u32(roc.astype(np.int64) + wrapped))
    uwant = plan_unprotect(want["dst"], got_off, got_size, ssrc, ctx, state, *_tag(tag_len))
    dst = dev.get(d_dst, (dst_bytes + 8,), np.uint8)
    assert (dst[:3] == 0x6B).all() and (dst[3 + dst_bytes:] == 0x6B).all()
    ugot = dict(ring=dst[3:3 + dst_bytes], state=dev.get(d_state, (S, 8), np.int32), sizes=dev.get(u_sizes, (n,), np.int32), status=dev.get(u_st, (n,), np.uint8),
                index=dev.get(u_idx, (n,), np.int64), stats=dev.get(u_stats, (16,), np.int32))
    _same(ugot, uwant, "unprotect in the chain")
    assert (ugot["status"][:k] == ref.OK).all() and (ugot["status"][k:] == ref.UN_RANGE).all()
    sent_last = (seq_base.astype(np.int64) & 0xFFFF) + np.clip(sc["counts"], 0, T) - 1
    for s in range(S):
        if sc["counts"][s] > 0:
            top = (int(ugot["state"][s, 1]) & 0xFFFFFFFF) << 16 | int(ugot["state"][s, 2])
            assert top == ((int(roc[s]) << 16) + int(sent_last[s])) & 0xFFFFFFFFFFFF, s
    # the frames in the ingest's tables
    assert (dev.get(i_st, (n,), np.uint8)[:k] == 0).all()
    oo, onb, cnt2 = dev.get(d_oo, (S, T), np.int64), dev.get(d_onb, (S, T), np.int32), dev.get(d_cnt2, (S,), np.int32)
    assert np.array_equal(cnt2, np.clip(sc["counts"], 0, T))
    ring = ugot["ring"]
    for s in range(S):
        for t in range(int(cnt2[s])):
            assert onb[s, t] == size and np.array_equal(ring[oo[s, t]:oo[s, t] + size], sc["frames"][s, t]), (s, t)
    enc.close()
    dec.close()
    return dict(S=S, ctx=ctx, wrapped=wrapped)
