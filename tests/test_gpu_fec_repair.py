"""Generic FEC, repair across calls, on the GPU (lc3plus_dec_batch_fec_repair; the nine kernels of liblc3plus_repair_hip.so).  Every output is held to equality
against the host plan (api.plan_fec_repair, itself held to the restatement of the rule in test_fec_repair_cpu.py): the three rec arrays, the statuses, stats, the
whole ring - arrival area, every slot of the history and the bytes between and behind them - fec_store, all metadata and the state, with guard elements behind
every array and the workspace filled with 0xA5 before every call.  The stores stay in device memory from call to call: only a call's datagrams are uploaded.
Stream and item counts on both sides of the wave and workgroup edges, both window sizes, packets of 12 ... 400 bytes at all four byte alignments with med_stride
an exact fit and one byte short, groups of 1, 5 and 16, a 48-bit mask, the 4 x 4 block with 1 ... 3 passes, twenty one-frame calls, heads that wrap 65535, the
launch counts of DESIGN 10s, the host conveniences, and sender to receiver over one-frame calls on one HIP stream against the CPU oracle's decode.  Device buffers
through ctypes (test_gpu_dec_varsize_device._Hip)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fec_ref
import fec_repair_ref as R
import hostile_frames as hf
from lc3_harness import synth_pcm
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_repair_hip.so")
GUARD, POISON = 16, 0xA5
SENTINEL = {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A}
KERNELS = ["lc3_rep_claim_kernel", "lc3_rep_copy_kernel", "lc3_rep_dist_kernel", "lc3_rep_fill_kernel", "lc3_rep_first_kernel", "lc3_rep_rebuild_kernel",
           "lc3_rep_report_kernel", "lc3_rep_settle_kernel", "lc3_rep_verdict_kernel"]
TYPES = dict(med_seq=np.int32, med_size=np.int32, fec_store=np.uint8, cell_seq=np.int32, cell_size=np.int32, cell_status=np.uint8, state=np.int32)


def _amd():
    import audio_codec_amd
    return audio_codec_amd


def launches(kernel):
    f = C.CDLL(LIB).lc3rep_launch_count
    f.restype, f.argtypes = C.c_longlong, [C.c_char_p]
    return f(kernel.encode())


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def decs():
    """decoder batches by their number of streams (the repair call reads it), made once"""
    made = {}

    def get(S):
        if S not in made:
            made[S] = _amd().DecBatch(S, 48000, 1, 10.0, 0, None, device=0)
        return made[S]
    yield get
    for d in made.values():
        d.close()


def _u32(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


class Session:
    """A receiver whose stores live in device memory, beside the host plan's: call() uploads the call's datagrams and item arrays alone, runs the kernels and the
    plan and holds everything the device holds equal to what the plan holds"""

    def __init__(self, dev, bat, S, garbage=None, **kw):
        api = _amd().api
        self.dev, self.bat, self.S, self.host = dev, bat, S, R.Receiver(api, S, **kw)
        if garbage is not None:
            rng = np.random.RandomState(garbage)
            for k in TYPES:
                if k != "state":
                    a = self.host.stores[k]
                    self.host.stores[k] = rng.randint(-(1 << 20), 1 << 20, a.shape).astype(a.dtype)
        st = self.host.stores
        self.ring = dev.put(np.concatenate([st["ring"], np.full(GUARD, 0x5A, np.uint8)]))
        self.d = {k: dev.put(np.concatenate([st[k].ravel(), np.full(GUARD, SENTINEL[dt], dt)])) for k, dt in TYPES.items()}
        self.work_bytes = api.fec_repair_work_bytes(S, st["med_slots"], st["fec_slots"])
        self.work = dev.put(np.full(self.work_bytes + 8, POISON, np.uint8))
        self.ssrc = dev.put(_u32(self.host.ssrc))

    def call(self, media=(), fec=(), passes=1, check=True):
        api, dev, st = _amd().api, self.dev, self.host.stores
        n, m, cells = len(media), len(fec), self.S * st["fec_slots"]
        ring, lists = self.host.lay(media, fec)
        assert dev.hip.hipMemcpy(C.c_void_p(self.ring), C.c_void_p(ring.ctypes.data), C.c_size_t(self.host.area), C.c_int(1)) == 0
        assert dev.hip.hipMemset(C.c_void_p(self.work), POISON, C.c_size_t(self.work_bytes)) == 0
        up = lambda a, dt: dev.put(np.array(a, dt)) if len(a) else None
        o, z, s, q = up(lists[0], np.int64), up(lists[1], np.int32), up(lists[2], np.int32), up(lists[3], np.int32)
        fo, fz, fs, fq = up(lists[4], np.int64), up(lists[5], np.int32), up(lists[6], np.int32), up(lists[7], np.int32)
        outs = dict(rec_dg_offsets=(cells, np.int64), rec_dg_sizes=(cells, np.int32), rec_seq=(cells, np.int32), item_status=(n, np.uint8), fec_status=(m, np.uint8),
                    stats=(16, np.int32))
        p = {k: dev.put(np.full(size + GUARD, SENTINEL[dt], dt)) for k, (size, dt) in outs.items()}
        before = {k: launches(k) for k in KERNELS}
        self.bat.fec_repair_device(n, self.ring, len(ring), o, z, s, q, m, fs, fo, fz, fq, self.ssrc, st["med_offset"], st["med_slots"], st["med_stride"], self.d["med_seq"],
                                   self.d["med_size"], self.d["fec_store"], st["fec_slots"], st["fec_stride"], self.d["cell_seq"], self.d["cell_size"], self.d["cell_status"],
                                   self.d["state"], p["rec_dg_offsets"], p["rec_dg_sizes"], p["rec_seq"], self.work, passes, p["item_status"], p["fec_status"], p["stats"],
                                   None, True)
        # the launches of DESIGN 10s: the item kernels only where the call has items, two kernels a pass
        for k in KERNELS:
            per_items = k in ("lc3_rep_first_kernel", "lc3_rep_dist_kernel", "lc3_rep_claim_kernel", "lc3_rep_copy_kernel")
            want = passes if k in ("lc3_rep_verdict_kernel", "lc3_rep_rebuild_kernel") else int(n + m > 0) if per_items else 1
            assert launches(k) == before[k] + want, k
        got = {}
        for k, (size, dt) in outs.items():
            a = dev.get(p[k], (size + GUARD,), dt)
            assert (a[size:] == SENTINEL[dt]).all(), ("an element behind the output was written", k)
            got[k] = a[:size]
        for k, dt in TYPES.items():
            a = dev.get(self.d[k], (st[k].size + GUARD,), dt)
            assert (a[st[k].size:] == SENTINEL[dt]).all(), ("an element behind the store was written", k)
            got[k] = a[:st[k].size].reshape(st[k].shape)
        a = dev.get(self.ring, (len(ring) + GUARD,), np.uint8)
        assert (a[len(ring):] == 0x5A).all(), "a byte behind the ring was written"
        got["ring"] = a[:len(ring)]
        assert (dev.get(self.work + self.work_bytes, (8,), np.uint8) == POISON).all(), "a byte behind the workspace was written"
        if check:
            want = self.host.call(lambda s_, *a_, **kw: api.plan_fec_repair(self.S, s_, *a_, poison_work=POISON, **kw), media, fec, passes)
            for k in R.OUTPUTS:
                w = np.asarray(want[k])
                bad = np.argwhere(got[k].reshape(w.shape) != w)
                assert len(bad) == 0, (k, "first differences at", bad[:4].tolist(), got[k].reshape(w.shape)[tuple(bad[0])], w[tuple(bad[0])])
        return got

    def rebuilt(self, r):
        return {(c // self.host.stores["fec_slots"], int(r["rec_seq"][c])) for c in np.flatnonzero(r["rec_dg_sizes"])}


SIZES = [12, 13] + list(range(20, 401, 19)) + [400]


def traffic(seed, S, per_call, calls, k, base=65500, loss=0.15, long_mask=False):
    """per call `per_call` media items over S streams, consecutive numbers from `base` (the heads wrap 65535), packets of SIZES bytes, parity over every k, a share
    of everything lost, the rest of each call shuffled, and every third call hostile items: a bad stream, a packet one byte too long for its slot, a short FEC item"""
    rng = np.random.RandomState(seed)
    sent, out, groups = [0] * S, [], {}
    for c in range(calls):
        media, fec = [], []
        for i in range(per_call):
            s = i % S
            sn = (base + 7 * s + sent[s]) & 0xFFFF
            pk = fec_ref.rtp_packet(rng, sn, SIZES[int(rng.randint(len(SIZES)))])
            sent[s] += 1
            group = groups.setdefault(s, [])
            group.append(pk)
            if rng.rand() > loss:
                media.append((s, sn, pk))
            if len(group) == k:
                if rng.rand() > loss:
                    fec.append((s, (sent[s] // k + 65533) & 0xFFFF, fec_ref.fec_packet(group, (sn - k + 1) & 0xFFFF, list(range(k)), long_mask)))
                group.clear()
        media = [media[i] for i in rng.permutation(len(media))]
        if c % 3 == 1:
            media += [(S, 5, media[0][2] if media else bytes(12)), (0, 9, bytes([0x80]) + bytes(400))]
            fec += [(0, 3, bytes(9))]
        out.append((media, fec))
    return out


# streams, media items a call, H, P, the group size, the byte alignment of the datagrams
SHAPES = [(1, 1, 16, 4, 1, 0), (3, 63, 16, 16, 5, 1), (3, 64, 64, 4, 16, 2), (65, 65, 16, 4, 1, 3), (257, 257, 64, 4, 1, 0), (65, 1025, 16, 16, 16, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_the_kernels_equal_the_host_plan(dev, decs, shape):
    S, per_call, H, P, k, align = shape
    calls = traffic(sum(shape), S, per_call, 3, k)
    area = max(sum(len(b) + 4 for _, _, b in media + fec) for media, fec in calls) + 64
    ses = Session(dev, decs(S), S, garbage=7, med_slots=H, med_stride=400, fec_slots=P, fec_stride=416, area=area, fill=0x3C, align=align, tail=48)
    seen, rebuilt = set(), 0
    for media, fec in calls:
        r = ses.call(media, fec, passes=2)
        rebuilt += len(ses.rebuilt(r))
        seen |= set(r["item_status"].tolist()) | set(r["fec_status"].tolist())
    if per_call >= 63:
        assert {R.STORED, R.OVERSIZE, R.DROPPED, R.SHORT} <= seen and rebuilt > 0


def test_a_48_bit_mask_and_the_block_in_one_two_and_three_passes(dev, decs):
    from test_fec_repair_cpu import block, packets, parity, three_pass_loss
    pk = packets(3, 500, 48)
    ses = Session(dev, decs(3), 3, med_slots=64)
    ses.call([(1, 500, pk[500])])
    ses.call([(1, 533, pk[533])], [(1, 0, parity(pk, 500, [0, 17, 33, 47], True))])
    r = ses.call([(1, 547, pk[547])])
    assert ses.rebuilt(r) == {(1, 517)} and r["stats"].tolist() == [1] + [0] * 15
    pk, fecs, _ = block(4)
    lost, gone, steps = three_pass_loss(4)
    media = [(0, sn, b) for sn, b in pk.items() if sn not in lost]
    fec = [(0, 40 + i, f) for i, f in enumerate(fecs) if i not in gone]
    for passes in (1, 2, 3):
        ses = Session(dev, decs(1), 1, med_slots=64, fec_slots=16, area=1 << 15)
        assert ses.rebuilt(ses.call(media, fec, passes)) == {(0, x) for x in set().union(*steps[:passes])}
    got = ses.rebuilt(ses.call(passes=4))                               # and a call without items: only the passes run
    assert not got


def test_twenty_one_frame_calls_with_all_state_in_device_memory(dev, decs):
    """four streams, a packet each a call, groups of 4 with the parity beside the closing packet, one loss a group, the heads crossing 65535: every lost packet is
    rebuilt, in the call its parity arrives in or - the last of a group - the call after"""
    S = 4
    ses = Session(dev, decs(S), S, fill=0xC3, med_stride=400)
    calls = traffic(99, S, S, 20, 4, base=65528, loss=0.0)
    got, lost = set(), set()
    for c, (media, fec) in enumerate(calls):
        drop = [x for x in media if x[1] == (65528 + 7 * x[0] + 4 * (c // 4) + (x[0] + c // 4) % 4) & 0xFFFF and c < 19]
        lost |= {(x[0], x[1]) for x in drop}
        got |= ses.rebuilt(ses.call([x for x in media if x not in drop], fec))
    assert got == lost and len(lost) == 19


def test_the_host_conveniences(decs):
    """DecBatch.fec_repair: uploaded, repaired, downloaded - with both lists, with media alone and with no item at all - is the plan, the stores chained"""
    from test_fec_repair_cpu import packets, parity
    api = _amd().api
    pk = packets(1, 100, 6, ssrc=0x01020305)                            # stream 1's in a Receiver
    a, b = R.Receiver(api, 2), R.Receiver(api, 2)
    bat = decs(2)
    for media, fec in (([(1, 100, pk[100]), (1, 102, pk[102])], []), ([(1, 103, pk[103])], [(1, 7, parity(pk, 100, [0, 1, 2, 3]))]), ([], [])):
        got = a.call(lambda st, *x, **kw: bat.fec_repair(st, *x, poison_work=POISON, **kw), media, fec, 2)
        want = b.call(lambda st, *x, **kw: api.plan_fec_repair(2, st, *x, **kw), media, fec, 2)
        for k in R.OUTPUTS:
            assert np.array_equal(got[k], want[k]), k
    assert a.packet_at(1, 101) == pk[101]


def test_every_repair_kernel_is_the_librarys_and_none_uses_scratch(dev, decs):
    from test_fec_repair_cpu import packets, parity
    pk = packets(1, 100, 4)
    ses = Session(dev, decs(1), 1)
    assert ses.rebuilt(ses.call([(0, sn, pk[sn]) for sn in (100, 101, 103)], [(0, 0, parity(pk, 100, [0, 1, 2, 3]))])) == {(0, 102)}
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    table = kernels(LIB, "gfx950")
    assert sorted(table) == KERNELS and all(v[3] == 0 for v in table.values()), table          # v[3]: the bytes of scratch
    assert all(launches(k) > 0 for k in KERNELS) and launches("lc3_fec_fill_kernel") == -1


@pytest.mark.parametrize("drops", [1, 2])
def test_sender_to_receiver_over_one_frame_calls(dev, drops):
    """Sixteen one-frame calls of four streams, 48k_10_128B, each call queued on one HIP stream with one wait at its end.  The sender: encode_device_packed, egress
    into a wire buffer, stamp, fec_encode (groups of 4, the state carried between two buffers), stamp of the FEC list.  The network: one media packet of every
    group never arrives (its size overwritten with -1 by an asynchronous copy).  The receiver: parse of the media and of the FEC datagrams, fec_repair with the
    history as its jitter buffer, parse of the history's slots by their offsets and med_size, probe, ingest at the position played - five calls behind, with a
    floor of one frame: what has not come by now is lost - and
    set_frame_counts + decode_device_packed.  One drop a group: the ingest reports no gap and the PCM equals the oracle's decode of the loss-free frames.  With a
    second drop in group 1 of every stream exactly those frames are concealed."""
    api = _amd().api
    geom = "48k_10_128B"
    fs, ms, hr, ch, sizes = hf.GEOMS[geom]
    S, T, N, size, k, D, H, P = 4, 16, hf.frame_len(fs, ms), int(sizes[0]), 4, 5, 16, 4
    room, pkt = 12, 12 + int(sizes[0])
    W, fstride = S * pkt, (12 + 14 + size + 15) & ~15
    F, ms_ = S * fstride, (pkt + 15) & ~15
    area = (W + F + 15) & ~15
    cap = area + S * H * ms_
    pcm_in = synth_pcm(S, T, N, fs, seed=43).reshape(S, T, ch, N)
    enc = _amd().Batch(S, fs, ch, ms, hr, [size * 800] * S, device=0)
    dec = _amd().DecBatch(S, fs, ch, ms, hr, None, device=0)
    i32, i64, u8 = (lambda n_, v=0: dev.put(np.full(n_, v, np.int32))), (lambda n_, v=0: dev.put(np.full(n_, v, np.int64))), (lambda n_, v=0: dev.put(np.full(n_, v, np.uint8)))
    buf = S * size + 64
    d_out, d_off, d_tot, d_nb, d_fl = u8(buf), i64((S, 1)), i64(1), i32((S, 1)), u8((S, 1))
    seq0 = (65530 + np.arange(S)).astype(np.int32)
    ssrc, fssrc = 0x7FFFFFF0 + 7 * np.arange(S), 0x100 + np.arange(S)
    d_seq, d_ssrc, d_fssrc, d_tsb = dev.put(seq0), dev.put(_u32(ssrc)), dev.put(_u32(fssrc)), dev.put(_u32(1000 * np.arange(S)))
    d_pt, d_fpt, d_sid = dev.put(np.full(S, 96, np.int32)), dev.put(np.full(S, 97, np.int32)), dev.put(np.arange(S, dtype=np.int32))
    d_ring = u8(cap + 8, 0x5A)
    d_fwire = d_ring + W
    p_route, p_seq, p_frame, p_off, p_size, p_flags = i32(S), i32(S), i32(S), i64(S), i32(S), u8(S)
    d_np, d_stats, d_cs, d_pst = i64(1), i32((S, 4)), u8((S, 1)), u8(S)
    e_work = dev.put(np.zeros(api.egress_work_bytes(S, 1) // 8 + 1, np.int64))
    d_group, d_fseq = dev.put(np.full(S, k, np.int32)), dev.put(np.full(S, 500, np.int32))
    f_n, f_route, f_seq, f_frame, f_off, f_size, f_flags, f_pst = i64(1), i32(S), i32(S), i32(S), i64(S), i32(S), u8(S), u8(S)
    f_state, f_acc = [i32((S, 8)), i32((S, 8))], [u8((S, 160)), u8((S, 160))]
    f_work = dev.put(np.full(api.fec_work_bytes(S, 1) + 8, POISON, np.uint8))
    f_dg = dev.put(W + fstride * np.arange(S, dtype=np.int64))
    i_stream, i_seq, i_off, i_nb = i32(S), i32(S), i64(S), i32(S)
    g_stream, g_seq, g_off, g_nb = i32(S), i32(S), i64(S), i32(S)
    med_seq, med_size, store = i32((S, H)), i32((S, H)), u8((S, P, fstride))
    cell_seq, cell_size, cell_status, state = i32((S, P)), i32((S, P)), u8((S, P)), i32((S, 4))
    r_off, r_size, r_seq = i64(S * P), i32(S * P), i32(S * P)
    r_work = dev.put(np.full(api.fec_repair_work_bytes(S, H, P) + 8, POISON, np.uint8))
    slots = dev.put(area + ms_ * np.arange(S * H, dtype=np.int64))
    h_stream, h_seq, h_off, h_nb = i32(S * H), i32(S * H), i64(S * H), i32(S * H)
    d_info = dev.put(np.zeros((S * H, ch, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci, d_cnt, d_ist, d_base, d_floor = i64((S, 1)), i32((S, 1)), i32((S, 1)), i32(S), i32((S, 4)), i32(S), i32(S, 1)
    d_pcm, d_st = dev.put(np.zeros((S, 1, ch, N), np.int16)), u8((S, 1))
    lost = np.zeros((S, T), bool)
    for s in range(S):
        for g in range(T // k):
            lost[s, k * g + (s + g) % k] = True
        if drops == 2:
            lost[s, k + (s + 2) % k] = True
    lost[:, T - 1] = False                                              # nothing arrives behind the last packet to move the head past it
    gone, zeros = dev.pin(np.full(1, -1, np.int32)), dev.pin(np.zeros(S, np.int32))
    frames, pcm, status, gaps = np.zeros((S, T, size), np.uint8), np.zeros((S, T, ch, N), np.int16), np.zeros((S, T), np.uint8), np.zeros((S, T), np.int32)
    s1 = dev.stream()
    dev.sync()
    for c in range(T + D):
        if c < T:
            d_in = dev.put(pcm_in[:, c:c + 1])
            base = dev.pin((seq0 + c).astype(np.int32))
            dev.copy_async(d_seq, base, s1)
            dev.copy_async(d_tsb, dev.pin(_u32(1000 * np.arange(S) + c * N)), s1)
            enc.encode_device_packed(d_in, 16, 1, d_out, buf, api.PACK_STREAM_MAJOR, None, None, d_off, d_tot, d_nb, d_fl, s1, sync=False)
            enc.egress_device(1, d_out, buf, d_off, d_nb, size, S, d_seq, p_route, p_seq, p_frame, p_off, p_size, d_np, e_work, d_fl, api.ENC_FL_PACK_CAP, None, None, 16,
                              api.PACK_STREAM_MAJOR, d_ring, W, room, 1, p_flags, None, None, d_stats, d_cs, s1, sync=False)
            enc.rtp_stamp_device(S, d_np, p_route, p_seq, p_frame, p_off, p_size, S, 1, d_ssrc, d_tsb, d_pt, N, d_ring, W, room, 0, p_flags, api.RTP_MARKER_NEVER, None, None,
                                 d_stats, d_pst, None, None, s1, sync=False)
            dev.copy_async(f_size, zeros, s1)                           # the entries behind n_fec are not written: no datagram there
            enc.fec_encode_device(S, d_np, p_route, p_frame, p_off, p_size, d_ring, W, S, 1, d_seq, d_group, d_fseq, d_fwire, F, fstride, S, f_n, f_route, f_seq, f_frame,
                                  f_off, f_size, f_work, room, 0, 12, d_pst, d_stats, None, f_state[c & 1], f_acc[c & 1], f_state[1 - (c & 1)], f_acc[1 - (c & 1)], 160,
                                  f_flags, None, d_fseq, None, s1, sync=False)
            enc.rtp_stamp_device(S, f_n, f_route, f_seq, f_frame, f_off, f_size, S, 1, d_fssrc, d_tsb, d_fpt, N, d_fwire, F, 12, 0, f_flags, api.RTP_MARKER_NEVER, None, None,
                                 None, f_pst, None, None, s1, sync=False)
            for s in np.flatnonzero(lost[:, c]):                        # stream-major, every cell SENT: packet s is stream s's
                dev.copy_async(p_size + 4 * int(s), gone, s1)
            dec.rtp_parse_device(S, d_ring, cap, p_off, p_size, S, d_ssrc, d_sid, i_stream, i_seq, i_off, i_nb, d_pt, 0, None, None, None, None, s1, sync=False)
            dec.rtp_parse_device(S, d_ring, cap, f_dg, f_size, S, d_fssrc, d_sid, g_stream, g_seq, g_off, g_nb, d_fpt, 0, None, None, None, None, s1, sync=False)
        n = S if c < T else 0
        dec.fec_repair_device(n, d_ring, cap, p_off, p_size, i_stream, i_seq, n, g_stream, g_off, g_nb, g_seq, d_ssrc, area, H, ms_, med_seq, med_size, store, P, fstride,
                              cell_seq, cell_size, cell_status, state, r_off, r_size, r_seq, r_work, 2, None, None, None, s1, sync=False)
        pos = c - D
        if pos >= 0:
            dev.copy_async(d_base, dev.pin((seq0 + pos).astype(np.int32)), s1)
            dec.rtp_parse_device(S * H, d_ring, cap, slots, med_size, S, d_ssrc, d_sid, h_stream, h_seq, h_off, h_nb, d_pt, 0, None, None, None, None, s1, sync=False)
            dec.probe_device(d_ring, cap, h_off, h_nb, size, S * H, d_info, api.PROBE_FULL, s1, sync=False)
            dec.ingest_device(S * H, h_stream, h_seq, h_off, h_nb, d_base, 1, d_oo, d_onb, d_ci, d_cnt, 16, d_info, d_floor, None, d_ist, None, s1, sync=False)
            dec.set_frame_counts(d_cnt)
            dec.decode_device_packed(d_ring, cap, d_oo, 1, d_pcm, d_onb, size, None, d_st, 16, s1, sync=False)
        dev.stream_sync(s1)                                             # the one wait of the call
        if c < T:
            out, off = dev.get(d_out, (buf,), np.uint8), dev.get(d_off, (S, 1), np.int64)
            for s in range(S):
                frames[s, c] = out[off[s, 0]:off[s, 0] + size]
        if pos >= 0:
            pcm[:, pos], status[:, pos] = dev.get(d_pcm, (S, 1, ch, N), np.int16)[:, 0], dev.get(d_st, (S, 1), np.uint8)[:, 0]
            gaps[:, pos] = dev.get(d_ci, (S, 1), np.int32)[:, 0] < 0
    hit = lost.reshape(S, T // k, k).sum(axis=2)
    want_gaps = lost & np.repeat(hit > 1, k, axis=1)
    assert np.array_equal(gaps.astype(bool), want_gaps) and (want_gaps.sum() == 0) == (drops == 1)
    o = hf.decode(geom, frames, np.where(want_gaps, 0, size), np.zeros((S, T), np.uint8))
    assert np.array_equal(status, o["status"]) and np.array_equal(status != 0, want_gaps)
    bad = np.argwhere((pcm != o["pcm"]).any(axis=(2, 3)))
    assert len(bad) == 0, ("first differing (stream, frame)", bad[:4].tolist())
    enc.close()
    dec.close()
