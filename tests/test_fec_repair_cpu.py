"""Generic FEC, repair across calls (include/lc3plus_batch.h "Generic FEC", REPAIR), no GPU: lc3plus_plan_fec_repair - the text the kernels run - against the rule
restated in tests/fec_repair_ref.py on every output and every store array, call after call; what the rule promises by construction (a group that spans calls is
repaired where lc3plus_plan_fec_recover leaves it MISSING, iterative passes reach the closure, every status); every refusal in the header's order; the plan in a
program of its own under the sanitizers; and the host round trip from plan_egress to plan_ingest over one-frame calls."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api, packet
import fec_ref
import fec_repair_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lc3plus_dec_batch_fec_repair", "lc3plus_plan_fec_repair", "lc3plus_fec_repair_work_bytes"]


def same(got, want, what=""):
    for k in R.OUTPUTS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


class Pair:
    """the plan and the restatement side by side, each over stores of its own, held equal after every call"""

    def __init__(self, S, **kw):
        self.S, self.plan, self.ref, self.calls = S, R.Receiver(packet, S, **kw), R.Receiver(packet, S, **kw), 0

    def garbage(self, seed):
        """everything but the state filled with noise, alike on both sides"""
        rng = np.random.RandomState(seed)
        for k in ("med_seq", "med_size", "cell_seq", "cell_size", "cell_status", "fec_store", "ring"):
            a = self.plan.stores[k]
            noise = rng.randint(-(1 << 20), 1 << 20, a.shape).astype(a.dtype)
            self.plan.stores[k], self.ref.stores[k] = noise, noise.copy()

    def call(self, media=(), fec=(), passes=1):
        got = self.plan.call(lambda st, *a, **kw: packet.plan_fec_repair(self.S, st, *a, poison_work=0xA5, **kw), media, fec, passes)
        want = self.ref.call(R.ref(self.S), media, fec, passes)
        same(got, want, "call %d" % self.calls)
        self.calls += 1
        return got

    def rebuilt(self, r):
        return {(c // self.plan.stores["fec_slots"], int(r["rec_seq"][c])) for c in np.flatnonzero(r["rec_dg_sizes"])}


def packets(seed, base, n, lo=20, hi=200, ssrc=0x01020304):
    rng = np.random.RandomState(seed)
    return {(base + i) & 0xFFFF: fec_ref.rtp_packet(rng, base + i, int(rng.randint(lo, hi + 1)), ssrc=ssrc) for i in range(n)}


def parity(pk, base, positions, long_mask=False):
    return fec_ref.fec_packet([pk[(base + i) & 0xFFFF] for i in positions], base & 0xFFFF, positions, long_mask)


def test_the_symbols_and_the_binding():
    L = audio_codec_amd.load_library()
    assert not [s for s in NEW if not hasattr(L, s) or s not in api.EXPORTS or s not in packet.PARAMS]
    assert callable(api.DecBatch.fec_repair_device) and callable(api.DecBatch.fec_repair) and callable(api.plan_fec_repair) and callable(api.fec_repair_work_bytes)
    # the repair call's constants are an enumeration in the header: the binding's and the restatement's are held to it, name by name
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    body = re.search(r"enum\s*\{([^}]*LC3PLUS_FEC_REPAIR_STATE_WORDS[^}]*)\}", text).group(1)
    header = {k: int(v) for k, v in re.findall(r"LC3PLUS_FEC_(\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", " ", body, flags=re.S))}
    assert header == dict(REPAIR_STATE_WORDS=4, STORED=0, STALE=10, DUPLICATE=11, OVERSIZE=12, EXPIRED=13, TWIN=14)
    for k, v in header.items():
        assert getattr(api, "FEC_" + k) == v, k
    assert (R.STORED, R.STALE, R.DUPLICATE, R.OVERSIZE, R.EXPIRED, R.TWIN, R.STATE_WORDS) == tuple(header[k] for k in ("STORED", "STALE", "DUPLICATE", "OVERSIZE", "EXPIRED",
                                                                                                              "TWIN", "REPAIR_STATE_WORDS"))
    assert api.FEC_REPAIR_OUTPUTS == R.OUTPUTS and api.FEC_REPAIR_STORES == R.STORES
    assert api.fec_repair_work_bytes(3, 16, 4) == 4 * (8 + 8 * 3 + 2 * 3 * 16 + 2 * 3 * 4) and api.fec_repair_work_bytes(3, 16, 4) % 8 == 0
    assert [api.fec_repair_work_bytes(*a) for a in ((0, 16, 4), (1, 8, 4), (1, 24, 4), (1, 2048, 4), (1, 16, 2), (1, 16, 512), (1 << 21, 1024, 4))] == [0] * 7


def test_a_group_of_four_over_one_packet_calls():
    """100 ... 103 with 101 lost, one packet a call, the parity beside 104: the old plan, which a call without FEC items cannot even make, finds the group MISSING in
    the one call it can make; the repair rebuilds 101 byte for byte in that call"""
    pk = packets(1, 100, 6)
    fp = parity(pk, 100, [0, 1, 2, 3])
    p = Pair(1)
    for sn in (100, 102, 103):
        r = p.call([(0, sn, pk[sn])])
        assert r["item_status"].tolist() == [R.STORED] and not r["rec_dg_sizes"].any()
    r = p.call([(0, 104, pk[104])], [(0, 7, fp)])
    assert r["fec_status"].tolist() == [R.RECOVERED] and r["stats"][R.RECOVERED] == 1 and p.rebuilt(r) == {(0, 101)}
    c = int(np.flatnonzero(r["rec_dg_sizes"])[0])
    a, n = int(r["rec_dg_offsets"][c]), int(r["rec_dg_sizes"][c])
    assert bytes(r["ring"][a:a + n]) == pk[101] == p.plan.packet_at(0, 101)
    r = p.call([(0, 105, pk[105])])
    assert not r["rec_dg_sizes"].any() and r["stats"].sum() == 0          # settled: no later call looks at the cell again
    # the old call on the closing call's lists
    ring, (o, z, s, q, fo, fz, fs, _) = R.Receiver(packet, 1).lay([(0, 104, pk[104])], [(0, 7, fp)])
    old = api.plan_fec_recover(1, ring, o, z, s, q, fs, fo, fz, [0x01020304], len(ring) - 512, 512, 64)
    assert old["status"].tolist() == [api.FEC_MISSING] and not old["rec_dg_sizes"].any()


@pytest.mark.parametrize("k", [2, 5, 16])
@pytest.mark.parametrize("lost", ["first", "middle", "last"])
def test_groups_of_other_sizes(k, lost):
    """the last member of a group lies ahead of the head when the parity comes with it gone: the next arrival moves the head and the cell settles then"""
    pk = packets(k, 65530, k + 1)
    out = {"first": 0, "middle": k // 2, "last": k - 1}[lost]
    p = Pair(1, med_slots=32)
    got = set()
    for i in range(k + 1):
        sn = (65530 + i) & 0xFFFF
        media = [] if i == out else [(0, sn, pk[sn])]
        fec = [(0, 65535, parity(pk, 65530, list(range(k))))] if i == k - 1 else []
        r = p.call(media, fec)
        got |= p.rebuilt(r)
        if fec:
            assert r["fec_status"].tolist() == [R.MISSING if out == k - 1 else R.RECOVERED]
    miss = (65530 + out) & 0xFFFF
    assert got == {(0, miss)} and p.plan.packet_at(0, miss) == pk[miss]
    assert p.plan.stores["state"].tolist() == [[3, (65530 + k) & 0xFFFF, 65535, 0]]


def test_a_48_bit_mask_and_parity_ahead_of_its_last_member():
    """positions 0, 17, 33, 47 under a long mask; the parity arrives a call before its last member and settles in the later call, counted in stats as a carried cell"""
    pos = [0, 17, 33, 47]
    pk = packets(3, 500, 48)
    p = Pair(2, med_slots=64, ssrc=[7, 0xFEDCBA98])
    p.call([(1, 500, pk[500])])
    p.call([(1, 533, pk[533])], [(1, 0, parity(pk, 500, pos, True))])
    assert p.plan.last["fec_status"].tolist() == [R.MISSING] and p.plan.last["stats"][R.MISSING] == 1
    r = p.call([(1, 547, pk[547])])
    want = bytearray(pk[517])
    want[8:12] = (0xFEDCBA98).to_bytes(4, "big")
    assert p.rebuilt(r) == {(1, 517)} and p.plan.packet_at(1, 517) == bytes(want)
    assert r["stats"].tolist() == [1] + [0] * 15 and p.plan.stores["cell_status"][1, 0] == R.RECOVERED
    assert p.plan.stores["state"][0].tolist() == [0, 0, 0, 0]             # stream 0 never had an item


def block(n, base=1000, seed=5):
    """an n x n block of numbers with row and column parity: the packets, the FEC packets (rows first) and their groups"""
    pk = packets(seed, base, n * n, 30, 90)
    groups = [[r * n + c for c in range(n)] for r in range(n)] + [[r * n + c for r in range(n)] for c in range(n)]
    return pk, [parity(pk, base, g, True) for g in groups], [{(base + i) & 0xFFFF for i in g} for g in groups]


def closure_passes(have, groups):
    """the numbers each synchronous pass rebuilds"""
    have, out = set(have), []
    while True:
        new = {next(iter(g - have)) for g in groups if len(g - have) == 1}
        if not new:
            return out
        out.append(new)
        have |= new


def three_pass_loss(n, base=1000):
    """the first loss pattern, media and parity, whose closure needs exactly three passes and repairs everything"""
    _, _, groups = block(n, base)
    nums = sorted(set().union(*groups))
    for m in range(3, 7):
        for lost in itertools.combinations(nums[:-1], m):
            for gone in itertools.combinations(range(len(groups)), 2):
                steps = closure_passes(set(nums) - set(lost), [g for i, g in enumerate(groups) if i not in gone])
                if len(steps) == 3 and set().union(*steps) == set(lost):
                    return set(lost), set(gone), steps
    raise AssertionError("no such pattern")


@pytest.mark.parametrize("n", [3, 4])
def test_a_block_with_row_and_column_parity_needs_three_passes(n):
    pk, fecs, groups = block(n)
    lost, gone, steps = three_pass_loss(n)
    media = [(0, sn, b) for sn, b in pk.items() if sn not in lost]
    fec = [(0, 40 + i, f) for i, f in enumerate(fecs) if i not in gone]
    kw = dict(med_slots=64, fec_slots=16, area=1 << 15)
    finals = {}
    for passes in (1, 2, 3):
        p = Pair(1, **kw)
        r = p.call(media, fec, passes)
        assert p.rebuilt(r) == {(0, x) for x in set().union(*steps[:passes])}
        finals[passes] = p.plan.stores
    for x in lost:
        j = x & 63
        a = finals[3]["med_offset"] + j * finals[3]["med_stride"]
        assert bytes(finals[3]["ring"][a:a + int(finals[3]["med_size"][0, j])]) == pk[x]
    # three calls of one pass, the last two without items, end where one call of three passes ends
    p = Pair(1, **kw)
    got = p.rebuilt(p.call(media, fec, 1)) | p.rebuilt(p.call(passes=1)) | p.rebuilt(p.call(passes=1))
    assert got == {(0, x) for x in lost}
    for k in R.STORES:
        if k != "ring":
            assert np.array_equal(p.plan.stores[k], finals[3][k]), k
    a = finals[3]["med_offset"]
    assert np.array_equal(p.plan.stores["ring"][a:], finals[3]["ring"][a:])


def test_what_the_closure_cannot_repair_stays_missing_and_expires():
    pk, fecs, groups = block(3)
    lost = {1000, 1001, 1003, 1004}                                       # a 2 x 2 square: every group that names one of them names two
    p = Pair(1, med_slots=16, fec_slots=8)
    r = p.call([(0, sn, b) for sn, b in pk.items() if sn not in lost], [(0, i, f) for i, f in enumerate(fecs)], 4)
    assert not r["rec_dg_sizes"].any() and sorted(r["fec_status"].tolist()) == [R.COMPLETE] * 2 + [R.MISSING] * 4
    later = packets(9, 1009, 12)
    for sn in range(1009, 1021):
        r = p.call([(0, sn, later[sn])])
        # 1000 falls behind a window of 16 under head 1016: its two groups expire there, 1001's at 1017, and 1003 / 1004's others with them
        want = {1016: 2, 1017: 1, 1019: 1}.get(sn, 0)
        assert r["stats"][R.EXPIRED] == want and r["stats"].sum() == want, sn
    assert (p.plan.stores["cell_status"] != R.MISSING).all()
    # once every number a cell names lies behind the window the cell itself is emptied, whatever its status
    more = packets(10, 1021, 8)
    for sn in range(1021, 1029):
        p.call([(0, sn, more[sn])])
    assert not p.plan.stores["cell_size"].any() and not p.plan.stores["cell_status"].any()


def test_one_call_that_holds_everything_is_the_recover_call():
    """no window collision, one pass, no packet lost at the top of its stream: statuses 0 ... 9 and the rebuilt bytes are plan_fec_recover's on the same items"""
    S, G, k = 3, 5, 4
    c, _ = fec_ref.recover_case(21, S, G, k, lambda s, g: [(s + g) % k] if (s + g) % 3 != 2 and not (g == G - 1 and (s + g) % k == k - 1) else
                                ([0, 2] if (s + g) % 2 else []), window=64, shuffle=True)
    old = api.plan_fec_recover(S, c["ring"], c["dg_offsets"], c["dg_sizes"], c["stream"], c["seq"], c["fec_stream"], c["fec_offsets"], c["fec_num_bytes"], c["ssrc"],
                               c["rec_offset"], c["rec_stride"], 64)
    assert {api.FEC_RECOVERED, api.FEC_COMPLETE, api.FEC_MISSING} <= set(old["status"].tolist())
    ring = np.concatenate([c["ring"], np.zeros(-len(c["ring"]) % 16 + S * 64 * 224, np.uint8)])
    st = packet.fec_repair_stores(S, ring, (len(c["ring"]) + 15) & ~15, 64, 224, 8, 240)
    count = {}
    fseq = [count.setdefault(int(s), []).append(0) or len(count[int(s)]) - 1 for s in c["fec_stream"]]
    args = (c["dg_offsets"], c["dg_sizes"], c["stream"], c["seq"], c["fec_stream"], c["fec_offsets"], c["fec_num_bytes"], fseq, c["ssrc"])
    new = packet.plan_fec_repair(S, st, *args)
    same(new, R.repair(S, st, *args))
    assert new["fec_status"].tolist() == old["status"].tolist() and new["stats"].tolist() == old["stats"].tolist()
    for f in np.flatnonzero(old["status"] == api.FEC_RECOVERED):
        cell = int(c["fec_stream"][f]) * 8 + (fseq[f] & 7)
        a, b, n = int(old["rec_dg_offsets"][f]), int(new["rec_dg_offsets"][cell]), int(old["rec_dg_sizes"][f])
        assert n == new["rec_dg_sizes"][cell] and old["rec_seq"][f] == new["rec_seq"][cell] and np.array_equal(old["ring"][a:a + n], new["ring"][b:b + n])


def test_the_one_difference_from_the_recover_call():
    """the same items in one call, the newest packet of the stream lost: the recover call rebuilds it, the repair call leaves the cell MISSING - the number lies
    ahead of the head, it may still arrive - and rebuilds it in the call whose arrival moves the head past it"""
    pk = packets(8, 300, 5)
    media, fec = [(0, sn, pk[sn]) for sn in (300, 301, 302)], [(0, 0, parity(pk, 300, [0, 1, 2, 3]))]
    ring, (o, z, s, q, fo, fz, fs, _) = R.Receiver(packet, 1).lay(media, fec)
    old = api.plan_fec_recover(1, ring, o, z, s, q, fs, fo, fz, [0x01020304], len(ring) - 512, 512, 64)
    assert old["status"].tolist() == [api.FEC_RECOVERED] and old["rec_seq"].tolist() == [303]
    p = Pair(1)
    r = p.call(media, fec)
    assert r["fec_status"].tolist() == [R.MISSING] and not r["rec_dg_sizes"].any() and p.plan.packet_at(0, 303) is None
    r = p.call([(0, 304, pk[304])])
    assert p.rebuilt(r) == {(0, 303)} and p.plan.packet_at(0, 303) == pk[303] and r["stats"][R.RECOVERED] == 1


def test_a_datagram_inside_the_history_is_out_of_range():
    """an item whose bytes touch the history - the call would read what it writes - is RANGE, media and FEC alike, one byte in is enough"""
    pk = packets(2, 40, 2)
    p = Pair(1)
    p.call([(0, 40, pk[40])])
    st = p.plan.stores
    a = st["med_offset"] + (40 & 15) * st["med_stride"]                   # the stored packet itself as a datagram; one that ends a byte inside the history
    n, edge = len(pk[40]), st["med_offset"] - 19
    args = ([a, edge], [n, 20], [0, 0], [41, 42], [0, 0], [a, edge], [n, 20], [1, 2], p.plan.ssrc)
    got = packet.plan_fec_repair(1, st, *args)
    same(got, R.repair(1, st, *args))
    assert got["item_status"].tolist() == [R.RANGE, R.RANGE] and got["fec_status"].tolist() == [R.RANGE, R.RANGE]
    ok = packet.plan_fec_repair(1, st, [edge - 1], [20], [0], [42], [], [], [], [], p.plan.ssrc)
    assert ok["item_status"].tolist() == [R.STORED]


def test_the_rec_list_is_a_datagram_list_for_the_parse():
    """a receiver that plays as packets arrive: the call's items and the parse of rec_dg_offsets / rec_dg_sizes over the ring the call left go to the ingest
    together.  The rebuilt packet's item wins its cell, and the cell points at the frame that was sent"""
    S, size, ssrc = 2, 40, np.array([0x01020304, 0x01020305])
    rng = np.random.RandomState(12)
    pk = [{sn: fec_ref.rtp_packet(rng, sn, 12 + size, ssrc=int(ssrc[s])) for sn in range(65533, 65533 + 6)} for s in range(S)]
    rx = R.Receiver(packet, S, ssrc=ssrc)
    lost = {0: 65534, 1: 65535}                                           # a middle member of each stream's group 65533 ... 65536
    played = 0
    for c in range(6):
        sn = 65533 + c
        media = [(s, sn & 0xFFFF, pk[s][sn]) for s in range(S) if lost[s] != sn]
        fec = [(s, 9, fec_ref.fec_packet([pk[s][x] for x in range(65533, 65537)], 65533, [0, 1, 2, 3])) for s in range(S)] if c == 3 else []
        r = rx.call(lambda st, *a, **kw: packet.plan_fec_repair(S, st, *a, **kw), media, fec)
        ring, (o, z, _, _, _, _, _, _) = rx.lay(media, fec)
        m = api.plan_rtp_parse(S, r["ring"], np.array(o, np.int64), np.array(z, np.int32), ssrc, np.arange(S), [96] * S)
        x = api.plan_rtp_parse(S, r["ring"], r["rec_dg_offsets"], r["rec_dg_sizes"], ssrc, np.arange(S), [96] * S)
        assert np.array_equal(x["status"] == 0, r["rec_dg_sizes"] > 0) and (x["status"][r["rec_dg_sizes"] == 0] == api.RTP_SHORT).all()
        if c != 3:
            assert not r["rec_dg_sizes"].any()
            continue
        items = {k: np.concatenate([m[k], x[k]]) for k in ("stream", "seq", "offsets", "num_bytes")}
        i = api.plan_ingest(S, 1, items["stream"], items["seq"], items["offsets"], items["num_bytes"], [65533, 65533], 4, 16)
        # of the group's four positions the call holds the last as its own item and the lost one as the rec list's; the other two arrived in earlier calls
        for s in range(S):
            t = lost[s] - 65533
            w = int(i["cell_item"][s, t])
            assert w >= len(m["stream"]) and i["num_bytes"][s, t] == size
            a = int(i["offsets"][s, t])
            assert bytes(r["ring"][a:a + size]) == pk[s][lost[s]][12:] and int(i["cell_item"][s, 3]) >= 0
            played += 1
    assert played == S


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_random_delivery_reaches_the_closure_however_it_is_cut(seed):
    """48 numbers under row parity over fours and column parity over every twelfth, a quarter of the media and a tenth of the parity lost, the rest in random order: with four passes a call
    and a window nothing leaves, the rebuilt numbers that never arrived are the closure's for every cut into calls (a packet that is merely late may be rebuilt
    before it arrives, and is then a DUPLICATE), and the history ends byte for byte the same"""
    rng = np.random.RandomState(seed)
    base, n = 65500, 48
    pk = packets(seed, base, n, 24, 120)
    groups = [list(range(g, g + 4)) for g in range(0, n, 4)] + [list(range(c, n, 12)) for c in range(12)]
    fecs = [(i, parity(pk, base, g, True), {(base + x) & 0xFFFF for x in g}) for i, g in enumerate(groups)]
    top = (base + n - 1) & 0xFFFF
    media = [(0, sn, b) for sn, b in pk.items() if sn == top or rng.rand() > 0.25]
    fec = [(0, (65530 + i) & 0xFFFF, f) for i, f, _ in fecs if rng.rand() > 0.1]
    want = R.closure({sn for _, sn, _ in media}, [g for i, _, g in fecs if any(q == (65530 + i) & 0xFFFF for _, q, _ in fec)])
    assert len(want) >= 3
    order = [("m", x) for x in media if x[1] != top] + [("f", x) for x in fec]
    order = [order[i] for i in rng.permutation(len(order))] + [("m", next(x for x in media if x[1] == top))]
    for cut in (1, 2, 7, len(order)):
        p = Pair(1, med_slots=64, fec_slots=32, area=1 << 15)
        got = set()
        for a in range(0, len(order), cut):
            part = order[a:a + cut]
            got |= p.rebuilt(p.call([x for k, x in part if k == "m"], [x for k, x in part if k == "f"], 4))
        for _ in range(3):
            got |= p.rebuilt(p.call(passes=4))
        arrived = {sn for _, sn, _ in media}
        assert {x for _, x in got} - arrived == want and (cut < len(order) or {x for _, x in got} == want), cut
        for x in pk:                                                  # the history ends the same whatever the cut: what arrived and what the closure yields
            assert p.plan.packet_at(0, x) == (pk[x] if x in arrived | want else None), (cut, x)


def test_garbage_stores_zeroed_state_and_a_quiet_stream():
    """four zero state words start a stream over stores of noise; a stream with no item keeps its state and its arrays, noise and all"""
    pk = packets(4, 65534, 6)
    p = Pair(3, fill=0xC3)
    p.garbage(11)
    quiet = {k: p.plan.stores[k][1].copy() for k in ("med_seq", "med_size", "cell_seq", "cell_size", "cell_status", "fec_store")}
    for i, sn in enumerate((65534, 65535, 1, 2)):
        fec = [(2, 65535 + i, parity(pk, 65534, [0, 1, 2, 3]))] if i == 3 else []
        r = p.call([(0, sn, pk[sn]), (2, sn, pk[sn])], fec)
    assert p.rebuilt(r) == {(2, 0)} and p.plan.packet_at(2, 0)[12:] == pk[0][12:] and p.plan.packet_at(0, 0) is None
    assert p.plan.stores["state"].tolist() == [[1, 2, 0, 0], [0, 0, 0, 0], [3, 2, 2, 0]]
    for k, v in quiet.items():
        assert np.array_equal(p.plan.stores[k][1], v), k
    assert (p.plan.stores["med_size"][0] > 0).sum() == 4 and (p.plan.stores["med_size"][2] > 0).sum() == 5


def test_every_status_by_construction():
    pk = packets(6, 200, 40, 40, 60)
    big = fec_ref.rtp_packet(np.random.RandomState(1), 300, 500)
    p = Pair(2, med_slots=16, med_stride=64, fec_slots=4, fec_stride=128, area=4096)
    # DROPPED, RANGE, SHORT and OVERSIZE on a media item; the FEC checks and OVERSIZE on an FEC item
    r = p.call([(0, 200, pk[200]), (5, 201, pk[201]), (0, 300, big), (0, 202, pk[202][:8]), (0, 200, pk[201])],
               [(0, 0, bytes(140)), (0, 1, bytes(10)), (3, 2, bytes(20)), (0, 3, bytes([0x80]) + bytes(19))])
    assert r["item_status"].tolist() == [R.STORED, R.DROPPED, R.OVERSIZE, R.SHORT, R.DUPLICATE]
    assert r["fec_status"].tolist() == [R.HEADER, R.SHORT, R.DROPPED, R.HEADER]
    assert p.plan.packet_at(0, 200) == pk[200]                              # of two copies in one call the lower index is stored
    long_fec = parity({300: big, 301: big}, 300, [0, 1])
    r = p.call([], [(0, 0, long_fec)])
    assert r["fec_status"].tolist() == [R.OVERSIZE] and len(long_fec) > 128
    # STALE and DUPLICATE against what is stored, in both spaces
    for sn in range(201, 220):
        p.call([(0, sn, pk[sn])])
    r = p.call([(0, 203, pk[203]), (0, 219, pk[220]), (0, 204, pk[204])])
    assert r["item_status"].tolist() == [R.STALE, R.DUPLICATE, R.DUPLICATE] and p.plan.packet_at(0, 219) == pk[219]
    r = p.call([], [(0, 50, parity(pk, 216, [0, 1])), (0, 54, parity(pk, 216, [2, 3]))])
    assert r["fec_status"].tolist() == [R.STALE, R.COMPLETE]
    r = p.call([], [(0, 54, parity(pk, 216, [0, 3]))])
    assert r["fec_status"].tolist() == [R.DUPLICATE]
    # TWIN: two parity packets over one loss; PARTIAL: a length recovery field that names more than the protection length; OVERFLOW: a lost packet too long
    # for its slot; EXPIRED: the parity of numbers that have left the window
    twin = parity(pk, 220, [0, 1, 2])
    part = bytearray(parity(pk, 224, [0, 1]))
    part[8:10] = (0x7000).to_bytes(2, "big")
    wide = {230: pk[230], 231: fec_ref.rtp_packet(np.random.RandomState(2), 231, 100)}
    r = p.call([(0, 220, pk[220]), (0, 222, pk[222]), (0, 224, pk[224]), (0, 230, pk[230]), (0, 232, pk[232])],
               [(0, 55, twin), (0, 56, twin), (0, 57, bytes(part)), (0, 58, parity(wide, 230, [0, 1]))])
    assert r["fec_status"].tolist() == [R.TWIN, R.RECOVERED, R.PARTIAL, R.OVERFLOW] and p.rebuilt(r) == {(0, 221)} and p.plan.packet_at(0, 221) == pk[221]
    r = p.call([], [(0, 59, parity(pk, 214, [0, 1, 8]))])
    assert r["fec_status"].tolist() == [R.EXPIRED] and r["stats"][R.EXPIRED] == 1
    # the late original of a rebuilt packet is a DUPLICATE and what was rebuilt stays
    other = bytearray(pk[221])
    other[20] ^= 0xFF
    r = p.call([(0, 221, bytes(other))])
    assert r["item_status"].tolist() == [R.DUPLICATE] and p.plan.packet_at(0, 221) == pk[221]


def test_an_exact_fit_and_one_byte_short():
    pk = {7: fec_ref.rtp_packet(np.random.RandomState(3), 7, 64), 8: fec_ref.rtp_packet(np.random.RandomState(4), 8, 65)}
    p = Pair(1, med_stride=64, fill=0x5A, tail=32)
    r = p.call([(0, 7, pk[7]), (0, 8, pk[8])])
    assert r["item_status"].tolist() == [R.STORED, R.OVERSIZE] and p.plan.packet_at(0, 7) == pk[7]
    a = p.plan.stores["med_offset"]
    rest = np.delete(r["ring"][a:], np.arange(7 * 64, 8 * 64))
    assert (rest == 0x5A).all()                                            # no byte outside the one slot is written


# ---- the refusals ----
def _valid():
    st = packet.fec_repair_stores(2, np.zeros(1024 + 2 * 16 * 64, np.uint8), 1024, 16, 64, 4, 64)
    v = packet._fec_repair_arrays(2, st, [0], [20], [0], [5], [1], [32], [20], [9], [1, 2], 1, None, packet.FEC_REPAIR_OPTIONAL)
    return dict(v, n_streams=2, hip_stream=None, sync=0)


def _code(v):
    try:
        packet._invoke(audio_codec_amd.load_library(), "lc3plus_plan_fec_repair", v, packet._host)
    except api.LC3Error as e:
        return e.code
    return 0


def test_refusals_in_the_headers_order():
    v = _valid()
    assert _code(v) == 0
    null = _code(dict(v, ring=None))
    rng = _code(dict(v, passes=0))
    assert null != 0 and rng != 0 and null != rng
    always = ("ring", "ssrc", "med_seq", "med_size", "fec_store", "cell_seq", "cell_size", "cell_status", "state", "rec_dg_offsets", "rec_dg_sizes", "rec_seq", "work")
    for k in always + ("dg_offsets", "dg_sizes", "stream", "seq", "fec_stream", "fec_offsets", "fec_num_bytes", "fec_seq"):
        assert _code(dict(v, **{k: None})) == null, k
        assert _code(dict(v, **{k: None}, passes=0)) == null, k             # NULLs are refused before ranges
    for k in ("item_status", "fec_status", "stats"):
        assert _code(dict(v, **{k: None})) == 0, k
    # an empty list needs no arrays
    assert _code(dict(v, n_items=0, dg_offsets=None, dg_sizes=None, stream=None, seq=None)) == 0
    assert _code(dict(v, n_fec=0, fec_stream=None, fec_offsets=None, fec_num_bytes=None, fec_seq=None)) == 0
    assert _code(dict(v, n_items=0, n_fec=0)) == 0
    bad = [dict(n_streams=0), dict(n_items=-1), dict(n_items=1 << 29), dict(n_fec=-1), dict(n_fec=1 << 29), dict(ring_capacity=-1), dict(med_offset=-16),
           dict(med_offset=1032), dict(med_slots=8), dict(med_slots=24), dict(med_slots=2048), dict(med_stride=0), dict(med_stride=72), dict(med_stride=(1 << 20) + 16),
           dict(fec_slots=2), dict(fec_slots=6), dict(fec_slots=512), dict(fec_stride=0), dict(fec_stride=40), dict(fec_stride=(1 << 20) + 16), dict(passes=0),
           dict(passes=5), dict(ring_capacity=1024 + 2 * 16 * 64 - 1), dict(med_offset=1040),
           # n_streams * H and n_streams * P of 2^31 under a ring_capacity such a history would fit: no other check refuses these
           dict(n_streams=1 << 21, med_slots=1024, med_stride=16, ring_capacity=1 << 40), dict(n_streams=1 << 23, fec_slots=256, med_stride=16, ring_capacity=1 << 40)]
    for kw in bad:
        assert _code(dict(v, **kw)) == rng, kw
    # overlaps: the FEC store inside the history, two metadata arrays in one
    ring = v["ring"]
    assert _code(dict(v, fec_store=ring[1024 + 64:])) == rng and _code(dict(v, fec_store=ring[:512])) == 0
    assert _code(dict(v, med_size=v["med_seq"])) == rng and _code(dict(v, cell_size=v["cell_seq"].reshape(-1)[1:])) == rng
    assert _code(dict(v, state=v["cell_status"])) == rng
    assert _code(dict(v, work=v["work"].view(np.uint8)[4:])) == rng
    L = audio_codec_amd.load_library()
    assert L.lc3plus_dec_batch_fec_repair(None, *[0] * (len(packet.PARAMS["lc3plus_dec_batch_fec_repair"]) - 1)) == null


# ---- the plan in a program of its own under the sanitizers ----
@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "audio_codec_amd", "csrc"), "repair_driver"])
    return os.path.join(ROOT, "audio_codec_amd", "_stub", "repair_plan_driver")


def _script(seed, S, H, P, calls, ms=96, fs=112, area=2048, passes=2):
    """a session drawn at random: every stream sends a packet a call, parity over every four, a fifth of everything lost, hostile items among them -> the text the
    driver reads and the calls for the restatement"""
    rng = np.random.RandomState(seed)
    rx = R.Receiver(packet, S, med_slots=H, med_stride=ms, fec_slots=P, fec_stride=fs, area=area, align=seed & 3)
    pk = [packets(100 * seed + s, 65520 + s, calls, 12, ms - 8) for s in range(S)]
    lines, log = ["%d %d %d %d %d %d %d %d" % (S, H, P, ms, fs, passes, rx.area, calls), " ".join(str(int(x)) for x in rx.ssrc)], []
    for c in range(calls):
        media, fec = [], []
        for s in range(S):
            sn = (65520 + s + c) & 0xFFFF
            if rng.rand() > 0.2:
                media.append((s, sn, pk[s][sn]))
            if c % 4 == 3 and rng.rand() > 0.2:
                fec.append((s, c // 4, parity(pk[s], 65520 + s + c - 3, [0, 1, 2, 3])))
        if c % 5 == 2:
            media.append((S + 1, 3, pk[0][65520 & 0xFFFF]))
            fec.append((0, 9, bytes(6)))
        ring, lists = rx.lay(media, fec)
        log.append((media, fec))
        lines.append("%d %d" % (len(media), len(fec)))
        for k in (0, 4):
            lines.append(" ".join("%d %d %d %d" % t for t in zip(*lists[k:k + 4])))
        lines.append(" ".join(str(int(x)) for x in ring[:rx.area]))
    return "\n".join(lines) + "\n", log, rx


@pytest.mark.parametrize("argv", [(1, 1, 16, 4, 13), (2, 3, 16, 4, 20), (3, 2, 32, 8, 9)])
def test_the_plan_under_sanitizers(driver, argv, tmp_path):
    """lc3plus_plan_fec_repair over a whole session in a program of its own under ASan + UBSan, the ring, the stores, the item arrays and the workspace heap blocks
    of their exact sizes: a clean exit, and every call's outputs and the final stores are the rule's"""
    text, log, rx = _script(*argv)
    path = tmp_path / "session.txt"
    path.write_text(text)
    p = subprocess.run([driver, "run", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    out = [dict((ln.split(":")[0], [int(x) for x in ln.split(":")[1].split()]) for ln in blk.strip().splitlines()) for blk in p.stdout.strip().split("\n\n")]
    assert len(out) == len(log) + 1
    for (media, fec), got in zip(log, out):
        want = rx.call(R.ref(rx.S), media, fec, 2)
        assert got["rc"] == [0]
        for k in ("rec_dg_offsets", "rec_dg_sizes", "rec_seq", "item_status", "fec_status", "stats"):
            assert got[k] == np.asarray(want[k]).ravel().tolist(), k
    for k in R.STORES:
        a = np.asarray(rx.stores[k]).ravel()
        assert out[-1][k] == (a[rx.area:] if k == "ring" else a).tolist(), k


def test_refusals_under_sanitizers(driver):
    p = subprocess.run([driver, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("refusals ok"), (p.stdout[-400:], p.stderr[-2000:])


# ---- the host round trip ----
def _chain(repair, calls=24, k=4, size=40, D=5):
    """plan_egress -> plan_rtp_stamp -> plan_fec_encode (its state carried) -> plan_rtp_stamp of the FEC list, one frame a call; one media packet of every group
    never arrives; the receiver parses what arrives and either repairs across calls - the history is its jitter buffer: every call it parses the history's slots
    by their offsets and med_size and plays position c - D - or, with the old call, recovers from each call's own lists and plays position c.  -> the ingest's
    gap count over the positions played and whether every played cell points at its frame's bytes"""
    rng = np.random.RandomState(8)
    S, N, room, H, P = 2, 480, 12, 16, 4
    seq0, ssrc, fssrc = np.array([65520, 7]), np.array([0x11111111, 0x22222222]), np.array([0x31111111, 0x32222222])
    frames = rng.randint(0, 256, (S, calls, size)).astype(np.uint8)
    drop = {(s, g * k + (s + g) % k) for s in range(S) for g in range(calls // k)} - {(s, calls - 1) for s in range(S)}
    stride, ms = 12 + 14 + size, (12 + size + 15) & ~15
    state, acc, fseq = np.zeros((S, api.FEC_STATE_WORDS), np.int32), np.zeros((S, 64), np.uint8), np.array([500, 600])
    rx = R.Receiver(packet, S, ssrc=ssrc, med_slots=H, med_stride=ms, fec_slots=P, fec_stride=(stride + 15) & ~15, area=1024)
    slots = rx.area + np.arange(S * H, dtype=np.int64) * ms
    gaps, right, played = 0, True, 0
    for c in range(calls + (D if repair else 0)):
        media, fec = [], []
        if c < calls:
            off = np.arange(S, dtype=np.int64).reshape(S, 1) * size
            e = api.plan_egress(S, frames[:, c].reshape(-1), off, np.full((S, 1), size, np.int32), seq0 + c, size, wire=np.zeros(S * (room + size), np.uint8), header_room=room)
            st = api.plan_rtp_stamp(e["pkt_route"], e["pkt_seq"], e["pkt_frame"], e["pkt_offset"], e["pkt_size"], ssrc, [c * N] * S, [96] * S, N, 1, e["wire"], room, 0,
                                    e["pkt_flags"], S, optional=("pkt_status",))
            f = api.plan_fec_encode(e["pkt_route"], e["pkt_frame"], e["pkt_offset"], e["pkt_size"], st["wire"], 1, seq0 + c, [k] * S, fseq, np.zeros(S * stride, np.uint8),
                                    stride, room, pkt_status=st["pkt_status"], n_packets=S, route_stats=e["stats"], state=state, acc=acc, acc_stride=64, max_fec_packets=S)
            state, acc, fseq = f["state"], f["acc"], f["next_fec_seq"]
            fs = api.plan_rtp_stamp(f["fec_route"], f["fec_seq"], f["fec_frame"], f["fec_offset"], f["fec_size"], fssrc, [c * N] * S, [97] * S, N, 1, f["fec_wire"], 12, 0,
                                    f["fec_flags"], f["n_fec"], optional=("pkt_status",))
            for p in range(S):
                s, a = int(e["pkt_route"][p]), int(e["pkt_offset"][p])
                if (s, c) not in drop:
                    media.append((s, None, bytes(st["wire"][a:a + int(e["pkt_size"][p])])))
            for q in range(f["n_fec"]):
                a = int(f["fec_offset"][q])
                fec.append((int(f["fec_route"][q]), None, bytes(fs["wire"][a:a + int(f["fec_size"][q])])))
        # the receiver: the datagrams into the arrival area, both parses over them
        ring, (o, z, _, _, fo, fz, _, _) = rx.lay(media, fec)
        o, z = np.array(o + fo, np.int64), np.array(z + fz, np.int32)
        if len(o):
            m = api.plan_rtp_parse(S, ring, o, z, ssrc, np.arange(S), [96] * S)
            g = api.plan_rtp_parse(S, ring, o, z, fssrc, np.arange(S), [97] * S)
            ok = g["status"] == 0
        if repair:
            if len(o):
                rx.last = api.plan_fec_repair(S, dict(rx.stores, ring=ring), o, z, m["stream"], m["seq"], g["stream"][ok], g["offsets"][ok], g["num_bytes"][ok],
                                              g["seq"][ok], ssrc, passes=2)
            else:
                rx.last = api.plan_fec_repair(S, rx.stores, [], [], [], [], [], [], [], [], ssrc, passes=2)
            rx.stores = {key: rx.last[key] for key in rx.stores}
            pos = c - D
            if pos < 0:
                continue
            x = api.plan_rtp_parse(S, rx.stores["ring"], slots, rx.stores["med_size"].reshape(-1), ssrc, np.arange(S), [96] * S)
            i = api.plan_ingest(S, 1, x["stream"], x["seq"], x["offsets"], x["num_bytes"], seq0 + pos, 1, 16)
            ring = rx.stores["ring"]
        else:
            pos, items = c, m
            if ok.any() and (m["status"] == 0).any():
                u = api.plan_fec_recover(S, np.concatenate([ring, np.zeros(S * 64, np.uint8)]), o, z, m["stream"], m["seq"], g["stream"][ok], g["offsets"][ok],
                                         g["num_bytes"][ok], ssrc, len(ring), 64, 64)
                x = api.plan_rtp_parse(S, u["ring"], u["rec_dg_offsets"], u["rec_dg_sizes"], ssrc, np.arange(S), [96] * S)
                items, ring = {key: np.concatenate([m[key], x[key]]) for key in ("stream", "seq", "offsets", "num_bytes")}, u["ring"]
            i = api.plan_ingest(S, 1, items["stream"], items["seq"], items["offsets"], items["num_bytes"], seq0 + pos, 1, 16)
        played += 1
        gaps += int((i["cell_item"][:, 0] < 0).sum())
        for s in range(S):
            if i["cell_item"][s, 0] >= 0:
                a = int(i["offsets"][s, 0])
                right = right and i["num_bytes"][s, 0] == size and bytes(ring[a:a + size]) == frames[s, pos].tobytes()
    return gaps, right, played, len(drop)


def test_host_round_trip_over_one_frame_calls():
    """24 one-frame calls, groups of 4, one loss per group: with the repair the ingest has no gap and every frame is the one sent; the same chain on the old
    recover call has a gap for every loss - the contrast this call exists for"""
    gaps, right, played, lost = _chain(True)
    assert (gaps, right, played) == (0, True, 24) and lost == 12
    gaps, right, played, lost = _chain(False)
    assert (gaps, right, played) == (lost, True, 24)
