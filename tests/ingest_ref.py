"""What packet ingest has to answer (test infrastructure, a plain helper beside frame_probe_ref.py): the rule of include/lc3plus_batch.h "Packet ingest" restated
in numpy from the header's text - sort the candidates of every cell by (rank, item) and take the first - and the item lists the tests run it on.

rule(case) -> dict with the keys of api.plan_ingest.  A case is a dict: n_streams, channels, n_frames, seq_bits, stream, seq, offsets, num_bytes [n], base
[n_streams], info [n, channels, 48] or None, floor [n_streams] or None.  Everything is drawn from np.random.RandomState integer draws, so the lists are
bit-reproducible."""
import functools
import itertools

import numpy as np

WORDS = 48
USED, DUPLICATE, LATE, EARLY, BAD_STREAM, EMPTY, REFUSED, INVALID = 1, 2, 4, 8, 16, 32, 64, 128
FI_CONCEALED, FI_INVALID, FI_LOST, FI_SKIPPED = 1, 2, 4, 8
KEYS = ("offsets", "num_bytes", "cell_item", "counts", "next_base", "stats", "item_status")
# the status words of an item's channels by what the probe found: accepted, refused in the first channel (a second one is skipped), refused in the second,
# invalid, lost
VERDICTS = {"ok": (0, 0), "refused0": (FI_CONCEALED, FI_CONCEALED | FI_SKIPPED), "refused1": (0, FI_CONCEALED), "invalid": (FI_CONCEALED | FI_INVALID,) * 2,
            "lost": (FI_CONCEALED | FI_LOST,) * 2}


def rule(c):
    S, T, bits, ch = c["n_streams"], c["n_frames"], c["seq_bits"], c["channels"]
    stream, nb, info = np.asarray(c["stream"], np.int64), np.asarray(c["num_bytes"], np.int64), c["info"]
    n = len(stream)
    mod = 1 << bits
    seq = np.asarray(c["seq"], np.int64) % mod
    base = np.asarray(c["base"], np.int64) % mod
    status = np.zeros(n, np.int64)
    bad = (stream < 0) | (stream >= S)
    status[bad] = BAD_STREAM
    st = np.asarray(info, np.int64)[:, :, 0] if info is not None else np.zeros((n, ch), np.int64)
    empty = ~bad & ((nb == 0) | ((st & FI_LOST) != 0).any(axis=1))
    status[empty] = EMPTY
    live = ~bad & ~empty
    s = np.where(bad, 0, stream)
    d = (seq - base[s]) % mod
    d = np.where(d >= mod // 2, d - mod, d)
    status[live & (d < 0)] = LATE
    status[live & (d >= T)] = EARLY
    cand = live & (d >= 0) & (d < T)
    rank = np.where((st == 0).all(axis=1), 0, np.where(((st & FI_INVALID) != 0).any(axis=1), 2, 1))
    out = dict(offsets=np.zeros((S, T), np.int64), num_bytes=np.zeros((S, T), np.int32), cell_item=np.full((S, T), -1, np.int32))
    idx = np.flatnonzero(cand)
    idx = idx[np.lexsort((idx, rank[idx]))]                      # by rank, then by place in the list
    cell = s[idx] * T + d[idx]
    _, first = np.unique(cell, return_index=True)
    win = idx[first]
    out["cell_item"].reshape(-1)[cell[first]] = win
    out["offsets"].reshape(-1)[cell[first]] = np.asarray(c["offsets"], np.int64)[win]
    out["num_bytes"].reshape(-1)[cell[first]] = nb[win]
    status[cand] = DUPLICATE
    status[win] = USED
    status[cand & (rank == 1)] |= REFUSED
    status[cand & (rank == 2)] |= INVALID
    filled = out["cell_item"] >= 0
    top = np.where(filled.any(axis=1), T - np.argmax(filled[:, ::-1], axis=1), 0)        # 1 + the highest filled t
    floor = np.zeros(S, np.int64) if c["floor"] is None else np.asarray(c["floor"], np.int64)
    counts = np.maximum(np.minimum(np.maximum(floor, 0), T), top)
    out["counts"] = counts.astype(np.int32)
    out["next_base"] = ((base + counts) % mod).astype(np.uint32).view(np.int32)
    gaps = np.array([int((~filled[k, :counts[k]]).sum()) for k in range(S)], np.int64)
    late = np.bincount(s[status == LATE], minlength=S)
    early = np.bincount(s[status == EARLY], minlength=S)
    out["stats"] = np.stack([counts, gaps, late, early], axis=1).astype(np.int32)
    out["item_status"] = status.astype(np.uint8)
    out["_rank"] = np.where(cand, rank, -1)
    return out


def _info(rng, verdicts, channels):
    """probe records with those verdicts: the status words set, every other word noise (the rule reads the status word alone)"""
    info = rng.randint(-1 << 31, 1 << 31, size=(len(verdicts), channels, WORDS)).astype(np.int32)
    for i, v in enumerate(verdicts):
        info[i, :, 0] = VERDICTS[v][:channels]
    return info


def _case(S, ch, T, bits, stream, seq, nb, base, offsets, verdicts=None, floor=None, rng=None):
    mod = 1 << bits
    c = dict(n_streams=S, channels=ch, n_frames=T, seq_bits=bits, stream=np.asarray(stream, np.int32),
             seq=(np.asarray(seq, np.int64) % mod).astype(np.uint32).view(np.int32), offsets=np.asarray(offsets, np.int64), num_bytes=np.asarray(nb, np.int32),
             base=(np.asarray(base, np.int64) % mod).astype(np.uint32).view(np.int32), info=_info(rng, verdicts, ch) if verdicts is not None else None,
             floor=None if floor is None else np.asarray(floor, np.int32))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def drawn(seed, S, T, n, ch, bits, with_info, with_floor=True, one_cell=False):
    """n items over S streams x T frames.  The bases lie just below 65536, so that every stream's sequence numbers pass 65535 inside the call (a wrap to 0 with 16
    bits, none with 32), the last stream's with 32 bits just below 2^32; distances from -3 to T + 2 with the four edges -1, 0, T - 1, T drawn most often; a few
    stream indices on either side of the range; a few sizes 0; floors from -2 to T + 3."""
    rng = np.random.RandomState(seed)
    mod = 1 << bits
    base = 65536 - 1 - rng.randint(0, max(T - 1, 1), size=S)
    if bits == 32:
        base[-1] = mod - 1 - rng.randint(0, max(T - 1, 1))
    stream = rng.randint(0, S, size=n)
    edges = np.array([-1, 0, T - 1, T])
    d = np.where(rng.randint(0, 3, size=n) == 0, edges[rng.randint(0, 4, size=n)], rng.randint(-3, T + 3, size=n))
    if one_cell:
        stream[:], d[:] = S - 1, T // 2
    seq = (base[stream] + d) % mod
    if not one_cell:
        stray = rng.randint(0, 12, size=n)
        stream = np.where(stray == 0, -1 - rng.randint(0, 2, size=n), np.where(stray == 1, S + rng.randint(0, 2, size=n), stream))
    nb = np.where(rng.randint(0, 15, size=n) == 0, 0, rng.randint(20, 401, size=n))
    offsets = rng.randint(0, 1 << 30, size=n).astype(np.int64) * 1021 + rng.randint(0, 4, size=n)
    verdicts = None
    if with_info:
        names = sorted(VERDICTS)
        verdicts = [names[k] if k < len(names) else "ok" for k in rng.randint(0, len(names) + 3, size=n)]
    floor = rng.randint(-2, T + 4, size=S) if with_floor else None
    return _case(S, ch, T, bits, stream, seq, nb, base, offsets, verdicts, floor, rng)


def pairs(bits, ch):
    """every pair of verdicts in one cell, in both list orders (the nine ordered pairs of ranks among them): one cell per pair, the first copy of all pairs, then
    the second ones"""
    rng = np.random.RandomState(77 + bits + ch)
    names = ("ok", "refused0", "refused1", "invalid")
    pr = list(itertools.product(names, names))
    T = 4
    S = (len(pr) + T - 1) // T
    base = 65533 + np.arange(S)
    stream = np.array([k // T for k in range(len(pr))] * 2)
    d = np.array([k % T for k in range(len(pr))] * 2)
    verdicts = [a for a, _ in pr] + [b for _, b in pr]
    n = len(stream)
    return _case(S, ch, T, bits, stream, base[stream] + d, rng.randint(20, 401, size=n), base, rng.randint(0, 1 << 40, size=n), verdicts, None, rng)


def edges(bits, T):
    """one stream, distances exactly -1, 0, T - 1 and T"""
    rng = np.random.RandomState(5)
    d = np.array([T, -1, T - 1, 0])
    return _case(1, 1, T, bits, np.zeros(4, int), 65535 + d, [40, 41, 42, 43], [65535], [1, 2, 3, 4], None, None, rng)


@functools.lru_cache(maxsize=None)
def cpu_lists():
    """name -> case, for the host plan; asserts that every status bit and every rank occurs in them"""
    out = {}
    for bits in (16, 32):
        for with_info in (False, True):
            tag = "%d_%s" % (bits, "info" if with_info else "plain")
            out["drawn_mono_" + tag] = drawn(1 + bits, 5, 7, 400, 1, bits, with_info)
            out["drawn_stereo_" + tag] = drawn(2 + bits, 4, 11, 500, 2, bits, with_info)
            out["one_cell_" + tag] = drawn(3 + bits, 3, 5, 120, 2, bits, with_info, one_cell=True)
            out["one_frame_" + tag] = drawn(4 + bits, 6, 1, 60, 1, bits, with_info)
            out["one_item_" + tag] = drawn(5 + bits, 2, 3, 1, 2, bits, with_info)
            out["no_floor_" + tag] = drawn(6 + bits, 3, 4, 50, 1, bits, with_info, with_floor=False)
        out["edges_%d" % bits] = edges(bits, 6)
        out["edges_one_frame_%d" % bits] = edges(bits, 1)
        out["pairs_mono_%d" % bits] = pairs(bits, 1)
        out["pairs_stereo_%d" % bits] = pairs(bits, 2)
    bits_seen, ranks_seen, floors = 0, set(), set()
    for name, c in out.items():
        r = rule(c)
        bits_seen |= int(np.bitwise_or.reduce(r["item_status"]))
        ranks_seen |= set(r["_rank"].tolist())
        if c["floor"] is not None:
            floors |= {"below" if f < 0 else "above" if f > c["n_frames"] else "inside" for f in c["floor"].tolist()}
        if name.startswith(("drawn", "pairs", "no_floor", "edges_1", "edges_3")):                 # the list passes 65535 inside the call
            low = np.asarray(c["seq"]).astype(np.int64) % 65536
            assert (low < 16).any() and (low > 65519).any(), name
    assert bits_seen == 255 and ranks_seen == {-1, 0, 1, 2} and floors == {"below", "inside", "above"}, (bits_seen, ranks_seen, floors)
    return out


@functools.lru_cache(maxsize=None)
def gpu_lists():
    """name -> case, for the kernels: sizes that fill neither waves nor workgroups evenly"""
    out = {}
    for bits in (16, 32):
        for with_info in (False, True):
            tag = "%d_%s" % (bits, "info" if with_info else "plain")
            out["3x4_" + tag] = drawn(11 + bits, 3, 4, 20, 2, bits, with_info)
            out["70x9_" + tag] = drawn(12 + bits, 70, 9, 1000, 1, bits, with_info)
            out["one_cell_" + tag] = drawn(13 + bits, 2, 3, 300, 2, bits, with_info, one_cell=True)
            out["2x130_" + tag] = drawn(14 + bits, 2, 130, 500, 1, bits, with_info)
    return out
