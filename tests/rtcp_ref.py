"""Reception reports restated (include/lc3plus_batch.h "Reception reports", "THE RULE", steps 1 to 7) in plain Python on plain integers, written from that text
and not from the C sources, and the item sets both test files use.  A case is a dict of stream, seq, timestamp, arrival [n], state [S, 10], ssrc, lsr, dlsr
[S] (lsr, dlsr: None for NULL); stats(case, make_report) gives what the calls give."""
import numpy as np

M = 0xFFFFFFFF
FLAGS, BASE_SEQ, MAX_SEQ, CYCLES, BAD_SEQ, RECEIVED, EXPECTED_PRIOR, RECEIVED_PRIOR, TRANSIT, JITTER = range(10)
STATE_WORDS = 10
STARTED = 1
DROPPED, COUNTED, JUMP, RESTART, REORDERED = range(5)
ST_COUNTED, ST_JUMP, ST_RESTART, ST_REORDERED = range(4)
STATS_WORDS = 4
BLOCK_BYTES = 24
MAX_DROPOUT, MAX_MISORDER = 3000, 100
KEYS = ("state", "blocks", "ext_seq", "item_status", "stream_stats")


def _i32(x):
    x &= M
    return x - (1 << 32) if x >> 31 else x


def _init_seq(w, q):
    w[BASE_SEQ] = w[MAX_SEQ] = q
    w[BAD_SEQ] = 65537
    w[CYCLES] = w[RECEIVED] = w[RECEIVED_PRIOR] = w[EXPECTED_PRIOR] = 0
    w[FLAGS] |= STARTED


def item(w, seq, timestamp, arrival):
    """steps 2 to 4 for one item of a valid stream on its state w (a list of ten ints, advanced in place) -> (status, ext_seq)"""
    q = seq & 0xFFFF
    first, status = False, COUNTED
    if not w[FLAGS] & STARTED:
        _init_seq(w, q)
        first = True
    else:
        udelta = (q - w[MAX_SEQ]) & 0xFFFF
        if udelta < MAX_DROPOUT:
            if q < w[MAX_SEQ]:
                w[CYCLES] = (w[CYCLES] + 65536) & M
            w[MAX_SEQ] = q
        elif udelta <= 65536 - MAX_MISORDER:
            if q == w[BAD_SEQ]:
                _init_seq(w, q)
                first, status = True, RESTART
            else:
                w[BAD_SEQ] = (q + 1) & 0xFFFF
                return JUMP, 0
        else:
            status = REORDERED
    w[RECEIVED] = (w[RECEIVED] + 1) & M
    transit = (arrival - timestamp) & M
    if first:
        w[TRANSIT], w[JITTER] = transit, 0
    else:
        d = (transit - w[TRANSIT]) & M
        w[TRANSIT] = transit
        ad = (0 - d) & M if _i32(d) < 0 else d
        w[JITTER] = (w[JITTER] + ad - ((w[JITTER] + 8 & M) >> 4)) & M
    ext = (w[CYCLES] + q - (65536 if q > w[MAX_SEQ] else 0)) & M
    return status, ext


def report(w, ssrc, lsr, dlsr):
    """step 6 for one stream -> its block's 24 bytes; the priors of w advanced"""
    if not w[FLAGS] & STARTED:
        return bytes(BLOCK_BYTES)
    expected = (w[CYCLES] + w[MAX_SEQ] - w[BASE_SEQ] + 1) & M
    lost = max(-0x800000, min(0x7FFFFF, _i32(expected - w[RECEIVED])))
    ei = _i32(expected - w[EXPECTED_PRIOR])
    li = _i32(((expected - w[EXPECTED_PRIOR]) & M) - ((w[RECEIVED] - w[RECEIVED_PRIOR]) & M))
    fraction = 0
    if ei != 0 and li > 0:
        num = li << 8
        fraction = min(255, num // ei if ei > 0 else -(num // -ei))          # truncating towards zero
    w[EXPECTED_PRIOR], w[RECEIVED_PRIOR] = expected, w[RECEIVED]
    words = (ssrc & M, (fraction & 255) << 24 | (lost & 0xFFFFFF), (w[CYCLES] + w[MAX_SEQ]) & M, w[JITTER] >> 4, lsr & M, dlsr & M)
    return b"".join(int(v).to_bytes(4, "big") for v in words)


def _words(a):
    return [int(v) & M for v in np.asarray(a).astype(np.int64).reshape(-1)]


def stats(c, make_report=True):
    """the whole rule -> dict of state [S, 10] int32, blocks [S, 24] uint8 (None without make_report), ext_seq [n] int32, item_status [n] uint8, stream_stats
    [S, 4] int32"""
    stream = [int(v) for v in np.asarray(c["stream"]).reshape(-1)]
    seq, ts, arr = _words(c["seq"]), _words(c["timestamp"]), _words(c["arrival"])
    S = np.asarray(c["state"]).reshape(-1, STATE_WORDS).shape[0]
    w = [_words(row) for row in np.asarray(c["state"]).reshape(-1, STATE_WORDS)]
    n = len(stream)
    ext, status, tally = [0] * n, [DROPPED] * n, [[0] * STATS_WORDS for _ in range(S)]
    for i in range(n):
        s = stream[i]
        if s < 0 or s >= S:
            continue
        status[i], ext[i] = item(w[s], seq[i], ts[i], arr[i])
        t = tally[s]
        t[ST_COUNTED] += status[i] != JUMP
        t[ST_JUMP] += status[i] == JUMP
        t[ST_RESTART] += status[i] == RESTART
        t[ST_REORDERED] += status[i] == REORDERED
    blocks = None
    if make_report:
        ssrc = _words(c["ssrc"])
        lsr = _words(c["lsr"]) if c.get("lsr") is not None else [0] * S
        dlsr = _words(c["dlsr"]) if c.get("dlsr") is not None else [0] * S
        blocks = np.frombuffer(b"".join(report(w[s], ssrc[s], lsr[s], dlsr[s]) for s in range(S)), np.uint8).reshape(S, BLOCK_BYTES).copy()
    u32 = lambda a, shape: np.array(a, np.uint32).reshape(shape).view(np.int32)
    return dict(state=u32(w, (S, STATE_WORDS)), blocks=blocks, ext_seq=u32(ext, (n,)), item_status=np.array(status, np.uint8),
                stream_stats=np.array(tally, np.int32).reshape(S, STATS_WORDS))


def block_fields(block):
    """a block's fields: ssrc, fraction, lost (signed), ext_high, jitter, lsr, dlsr"""
    b = bytes(bytearray(np.asarray(block, np.uint8).tolist()))
    lost = int.from_bytes(b[5:8], "big")
    return dict(ssrc=int.from_bytes(b[0:4], "big"), fraction=b[4], lost=lost - (1 << 24) if lost >> 23 else lost, ext_high=int.from_bytes(b[8:12], "big"),
                jitter=int.from_bytes(b[12:16], "big"), lsr=int.from_bytes(b[16:20], "big"), dlsr=int.from_bytes(b[20:24], "big"))


# ---- item sets ----
def case(stream, seq, timestamp, arrival, n_streams=None, state=None, lsr=True):
    stream = np.asarray(stream, np.int64)
    S = int(n_streams if n_streams is not None else stream.max() + 1)
    k = np.arange(S, dtype=np.int64)
    return dict(stream=stream.astype(np.int32), seq=np.asarray(seq, np.int64), timestamp=np.asarray(timestamp, np.int64) & M, arrival=np.asarray(arrival, np.int64) & M,
                state=np.zeros((S, STATE_WORDS), np.int64) if state is None else np.asarray(state, np.int64).reshape(S, STATE_WORDS),
                ssrc=(0x7FFFFF00 + 977 * k) & M, lsr=(0xC0DE0000 + k) & M if lsr else None, dlsr=(65536 * 3 + 7 * k) & M if lsr else None)


# one stream each: the sequence numbers, in arrival order
PATTERNS = {
    "one": [7],
    "wrap": [65534, 65535, 0, 1],
    "reordered_across_wrap": [65534, 0, 65535, 1],
    "duplicate": [10, 11, 11, 12],
    "dropout_2999": [100, 3099, 3100],                              # udelta = 2999: in order
    "dropout_3000": [100, 3100, 101],                               # udelta = 3000: a jump, then in order
    "misorder_65436": [100, 0, 101],                                # udelta = 65436 = 65536 - 100: a jump
    "misorder_65437": [100, 1, 101],                                # udelta = 65437: reordered
    "misorder_wrapped": [65500, 65400, 65401],                      # udelta = 65436 through the wrap of the difference
    "jump_then_successor": [100, 5000, 5001, 5002],                 # a restart
    "jump_then_other": [100, 5000, 7000, 101, 7001, 7002],          # two jumps, in order, then the second jump's successor: a restart
    "jump_then_same": [100, 5000, 5000, 102],                       # the jump again is no successor
    "restart_at_wrap": [100, 65535, 0, 1],                          # BAD_SEQ wraps to 0
    "seq_above_16_bits": [0x12340005, 6 - 65536, 7],                # only the low 16 bits count
}


def patterns(names=None, ts_step=480):
    """the named patterns, one stream each, interleaved round-robin; timestamps follow the sequence numbers and arrivals wander around them"""
    names = list(PATTERNS) if names is None else list(names)
    rows = []
    for s, nm in enumerate(names):
        for k, q in enumerate(PATTERNS[nm]):
            ts = 1000 * s + ts_step * (q & 0xFFFF)
            rows.append((k, s, q, ts, ts + 5000 + ((k * 37 + s * 11) % 97) * (1 if k & 1 else -1)))
    rows.sort(key=lambda r: (r[0], r[1]))
    c = case([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], len(names))
    return c, {nm: s for s, nm in enumerate(names)}


def transits():
    """arrival - timestamp across 2^31 and 2^32 and a d of exactly 0x80000000, three streams"""
    ts0 = [0xFFFFFF00, 0x00000100, 0x7FFFFFF0, 0x80000010, 5]                           # stream 0: the difference wraps both ways
    ar0 = [0x00000010, 0xFFFFFFF0, 0x80000020, 0x7FFFFFF0, 0x80000005]
    ts1, ar1 = [0, 0, 0, 0], [0, 0x80000000, 0, 0x7FFFFFFF]                              # stream 1: d = 0x80000000, -0x80000000 mod 2^32, 0x7FFFFFFF
    ts2, ar2 = [0x80000000, 0x80000001], [0x7FFFFFFF, 0x80000002]                        # stream 2: transit -1 then 1
    stream = [0] * 5 + [1] * 4 + [2] * 2
    order = np.argsort(np.array([0, 3, 6, 9, 12, 1, 4, 7, 10, 2, 5]), kind="stable")
    col = lambda a: np.array(a, np.int64)[order]
    return case(col(stream), col([1, 2, 3, 4, 5, 1, 2, 3, 4, 1, 2]), col(ts0 + ts1 + ts2), col(ar0 + ar1 + ar2), 3)


def started(base, max_seq, cycles, received, expected_prior=0, received_prior=0, transit=0, jitter=0, bad=65537, flags=1):
    return [flags, base, max_seq, cycles, bad, received, expected_prior, received_prior, transit, jitter]


def crafted_states():
    """reports from crafted state blocks, one stream each: (case, the streams by name).  Streams 0 ... 5 receive nothing in the call, 6 receives one JUMP"""
    rows = dict(
        lost_below=started(10, 20, 0, 0x01000000),                      # expected 11, received 2^24: lost far below -0x800000
        lost_above=started(0, 5, 0x01000000, 3),                        # expected 2^24 + 6: lost above 0x7FFFFF
        lost_edges=started(0, 0xFFFF, 0x7F0000, 1),                     # expected 0x800000, received 1: lost = 0x7FFFFF exactly
        fraction_cap=started(0, 99, 0, 50, expected_prior=90, received_prior=50),        # ten expected, none received: 256 -> 255
        fraction_half=started(0, 99, 0, 95, expected_prior=90, received_prior=90),       # ten expected, five received: 128
        negative_interval=started(0, 9, 0, 5, expected_prior=30, received_prior=40),     # ei = -20, li = 15: -192 -> 0x40
        jump_only=started(0, 99, 0, 100, expected_prior=100, received_prior=100, jitter=0x123),
        not_started=[0] * STATE_WORDS,
        flag_bits=started(5, 5, 0, 1, flags=0x7FFFFFF1),
        not_started_bits=[6, 1, 2, 3, 4, 5, 6, 7, 8, 9],                # bit 0 clear: whatever the block holds, the source has not started
    )
    names = list(rows)
    s = names.index("jump_only")
    c = case([s, names.index("not_started_bits"), -1], [40000, 9, 9], [0, 0, 0], [0, 77, 0], len(names), state=[rows[k] for k in names])
    return c, {nm: k for k, nm in enumerate(names)}


def traffic(seed, n_streams, frames, silent=(), bad_items=0.02, with_faults=True, ts_step=480, clean_start=False):
    """what a receiver sees: every stream sends `frames` packets from a base of its own (some just below the wrap), the network loses, duplicates and reorders
    some and delays each by a wandering amount, a few senders restart at another sequence number; the streams interleave in arrival order.  Streams in `silent`
    send nothing.  bad_items: the share of items of no stream (-1, n_streams, far outside) scattered through.  clean_start: a stream's first packet arrives
    first (no packet reordered in front of it)"""
    rng = np.random.RandomState(seed)
    rows = []
    for s in range(n_streams):
        if s in silent:
            continue
        base = int(rng.choice([0, 65536 - frames // 2, rng.randint(65536), 65535]))
        ts0, delay = int(rng.randint(1 << 32)), int(rng.randint(1 << 32))
        restart_at = rng.randint(2, frames) if with_faults and frames > 4 and rng.rand() < 0.2 else -1
        shift, t_arr = 0, float(rng.rand())
        for k in range(frames):
            if k == restart_at:
                shift = int(rng.randint(3000, 60000))
            q = base + k + shift
            t_arr += 1.0
            if k and rng.rand() < (0.07 if with_faults else 0.1):     # lost
                continue
            late = 0.0
            if k and not clean_start and with_faults and rng.rand() < 0.05:
                late = float(rng.randint(1, 4)) + 0.5                 # reordered behind later packets
            elif k > 1 and clean_start and with_faults and rng.rand() < 0.05:
                late = 1.5
            ts = ts0 + ts_step * (k + shift)
            arrival = ts + delay + int(rng.randint(-200, 200)) + int(late * ts_step)
            rows.append((t_arr + late, s, q, ts, arrival))
            if with_faults and rng.rand() < 0.03:                      # duplicated
                rows.append((t_arr + late + 0.25, s, q, ts, arrival + 31))
    n_bad = int(len(rows) * bad_items)
    for _ in range(n_bad):
        rows.append((float(rng.rand()) * (frames + 1), int(rng.choice([-1, n_streams, n_streams + 5, -7, 1 << 30])), int(rng.randint(65536)), 0, 0))
    rows.sort(key=lambda r: r[0])
    return case([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], n_streams)


def one_stream(n, seed=1, n_streams=1, stream=0):
    """n items of one stream (of n_streams), in order with a few losses, duplicates and reordered packets"""
    rng = np.random.RandomState(seed)
    q = 65500 + np.cumsum(rng.choice([1, 1, 1, 1, 2, 0], size=n))
    swap = np.flatnonzero(rng.rand(n - 1) < 0.05) if n > 1 else []
    for k in swap:
        q[k], q[k + 1] = q[k + 1], q[k]
    ts = 480 * q
    return case(np.full(n, stream), q, ts, ts + 12345 + rng.randint(-300, 300, size=n), n_streams)


def cpu_sets():
    """the generated sets of the host tests: name -> case"""
    out = {"patterns": patterns()[0], "transits": transits(), "crafted_states": crafted_states()[0]}
    for nm in PATTERNS:
        out["pattern_" + nm] = patterns([nm])[0]
    out["traffic_5x40"] = traffic(1, 5, 40)
    out["traffic_65x30_silent"] = traffic(2, 65, 30, silent=(0, 7, 64))
    out["traffic_300x8"] = traffic(3, 300, 8)
    out["traffic_2x700"] = traffic(4, 2, 700)
    out["one_stream_129"] = one_stream(129)
    out["one_stream_of_three"] = one_stream(70, 2, 3, 1)
    out["all_dropped"] = case([-1, 5, 2], [1, 2, 3], [0, 0, 0], [0, 0, 0], 2)
    return out


def split(c, k):
    """the case cut in two at item k"""
    cut = lambda lo, hi: dict(c, **{key: c[key][lo:hi] for key in ("stream", "seq", "timestamp", "arrival")})
    return cut(0, k), cut(k, len(c["stream"]))
