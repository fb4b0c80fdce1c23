"""Hostile payloads for the decoder (test infrastructure, a plain helper beside signal_classes.py): frames the bitstream parser has to refuse, one class per
"conceal this frame" decision of the reference (R/dec_entropy.c:120-270, R/ari_codec.c:204-509; LC3O_REJ_* in oracle/lc3_oracle.h), and frames it accepts
although no encoder would write them.

Payload sources.  pool(fs, ms, hr, size) draws random payloads (np.random.RandomState integer draws only, so everything here is bit-reproducible) and classes
each by the CPU oracle's verdict: accepted ("H") or refused for reason x ("R_x", OracleDecoder.last_reject).  Where a field edit reaches a reason directly
it is crafted instead of searched for - the side-information bits are written at the positions dec_side reads them (side_fields) into an accepted payload:
the joint SNS index at its first invalid value and all ones in both forms, the first three bytes FF FF FF with and without a TNS flag, the bandwidth and
lastnz fields at their first invalid value, an order-8 TNS filter (refused at the short frame lengths), the global gain at 0 and 255 and, on a genuine
full-scale frame, 28 steps up.  The oracle classes the crafted
payloads like the drawn ones; tests/test_hostile_frames_cpu.py counts what the streams really hold.  Genuine frames ("G") are the oracle encoder's on
lc3_harness.synth_pcm at the same size.

streams(geom) -> (frames [B, T, stride], sizes [B, T], bfi [B, T], kind [B, T], reason [B * channels, T]), one stream per pattern (PATTERNS)."""
import collections
import functools
import math

import numpy as np

from lc3_harness import Oracle, OracleDecoder, synth_pcm

T = 24
CUT = 13                                           # the second call of the two-call tests starts here
G, H, R, FLAG, EMPTY = 0, 1, 2, 3, 4               # kind: genuine, accepted random, refused, flagged (bfi = 1), size 0
# LC3O_REJ_* (oracle/lc3_oracle.h); test_hostile_frames_cpu.test_reason_codes_are_the_oracle_s holds them against the library's own names and count
REJ_NAMES = ("none", "bandwidth", "lastnz", "sns_index_25", "sns_index_24", "tns_order", "tns_reader", "tns_symbol", "overlap", "spec_symbol", "escape_14", "nres")
(REJ_BANDWIDTH, REJ_LASTNZ, REJ_SNS_25, REJ_SNS_24, REJ_TNS_ORDER, REJ_TNS_READER, REJ_TNS_SYMBOL, REJ_OVERLAP, REJ_SPEC_SYMBOL, REJ_ESCAPE_14,
 REJ_NRES) = REASONS = tuple(range(1, len(REJ_NAMES)))
BW_BITS = (0, 1, 2, 2, 3, 0)                       # by fs_idx (R/constants.c bw_bits)

# name -> fs, frame_ms, hrmode, channels, stream-frame bytes of every stream (PATTERNS order); the mixed geometry's last stream changes its size at frame CUT
GEOMS = collections.OrderedDict([
    ("48k_10_20B", (48000, 10.0, 0, 1, (20,) * 7)),                            # minimum size: the TNS reader collision; LDS-staged parser
    ("48k_10_128B", (48000, 10.0, 0, 1, (128,) * 7)),                          # largest LDS-staged frame
    ("48k_10_mixed", (48000, 10.0, 0, 1, (128, 80, 130, 400, 20, 128, 20, (80, 400)))),   # maximum above 128: the global-memory parser, largest frame
    ("24k_5_30B", (24000, 5.0, 0, 1, (30,) * 7)),                              # the bandwidth field can be invalid; maxlag 4
    ("16k_2p5_20B", (16000, 2.5, 0, 1, (20,) * 7)),                            # one filter, ylen 40
    ("48k_hr_156B", (48000, 10.0, 1, 1, (156,) * 7)),                          # 21 escape levels; global parser
    ("96k_2p5_hr_62B", (96000, 2.5, 1, 1, (62,) * 7)),                         # high resolution on the LDS parser
    ("96k_10_hr_625B", (96000, 10.0, 1, 1, (625,) * 7)),                       # the large layout, the largest frame there is
    ("48k_10_stereo_161B", (48000, 10.0, 0, 2, (161,) * 7)),                   # 81 + 80 bytes: rejections in channel 0 only, channel 1 only, both
])
# one stream per pattern.  In the stereo geometry a refused frame is refused in channel 0 ("0"), channel 1 ("1") or both ("b").
PATTERNS = ("r_first", "r_behind_g", "r_behind_h", "all_h", "alternating", "burst", "h_r1", "size_change")
STEREO_WHERE = {"r_first": "0", "r_behind_g": "1", "r_behind_h": "0", "alternating": "01b", "burst": "0", "h_r1": "1"}
BURST = (8, (R, FLAG, EMPTY, R, R, FLAG, EMPTY, R, R))      # nine losses from frame 8: nbLost passes 4 and 8, the burst crosses frame CUT; frame 17 is H


def frame_len(fs, ms):
    return int(fs * ms / 1000)


def coded_lines(fs, ms, hr):
    n = frame_len(fs, ms)
    return n if hr else min(n, int(400 * ms / 10))


def fs_index(fs):
    return 5 if fs == 96000 else 4 if fs == 48000 else fs // 8000 - 1


def max_lag(ms):
    return 8 if ms == 10.0 else 4


def channel_sizes(size, channels):
    return [size // channels + (c < size % channels) for c in range(channels)]


# ---- the side information's bit positions (R/dec_entropy.c:120-270): backward bit q is bit (q & 7) of byte nbytes - 1 - (q >> 3) ----------------------------
def get_bits(p, q, n):
    return sum(((int(p[len(p) - 1 - ((q + i) >> 3)]) >> ((q + i) & 7)) & 1) << i for i in range(n))


def put_bits(p, q, n, v):
    for i in range(n):
        j = len(p) - 1 - ((q + i) >> 3)
        p[j] = (int(p[j]) & ~(1 << ((q + i) & 7))) | (((v >> i) & 1) << ((q + i) & 7))


def side_fields(p, fs, ms, hr):
    """{field: (first backward bit, bits)} as dec_side walks this payload: the TNS flags depend on the bandwidth it holds, the index on the msb bit"""
    f, q = collections.OrderedDict(), 0

    def take(name, n):
        nonlocal q
        f[name] = (q, n); q += n
    bwb = 0 if hr else BW_BITS[fs_index(fs)]
    take("bw", bwb)
    bw = get_bits(p, 0, bwb) if bwb else fs_index(fs)
    take("lastnz", int(math.ceil(math.log2(coded_lines(fs, ms, hr) / 2))))
    take("lsb", 1); take("gg", 8); take("tns0", 1)
    if not (bw < 3 or ms == 2.5):
        take("tns1", 1)
    take("ltpf", 1); take("sns_lf", 5); take("sns_hf", 5); take("msb", 1)
    msb = get_bits(p, *f["msb"])
    take("gain", 1 + msb); take("ls", 1); take("index", 25 - msb)
    return f


def edit(p, fs, ms, hr, **values):
    """a copy of payload p with the named side-information fields set, in the order given (the positions are found again after every field)"""
    p = p.copy()
    for k, v in values.items():
        if k == "head":
            p[:len(v)] = v
            continue
        f = side_fields(p, fs, ms, hr)
        if k in f:
            put_bits(p, f[k][0], f[k][1], v)
    return p


def crafts(fs, ms, hr, size):
    """name -> field edits; the oracle says what each one gives"""
    c = collections.OrderedDict()
    c["sns25_first"] = dict(msb=0, index=33460056); c["sns25_ones"] = dict(msb=0, index=(1 << 25) - 1)
    c["sns24_first"] = dict(msb=1, index=16708096); c["sns24_ones"] = dict(msb=1, index=(1 << 24) - 1)
    c["ff3"] = dict(tns0=0, tns1=0, head=(255, 255, 255)); c["ff3_tns"] = dict(tns0=1, head=(255, 255, 255))
    bwb = 0 if hr else BW_BITS[fs_index(fs)]
    if fs_index(fs) + 1 < 1 << bwb:
        c["bw_first"] = dict(bw=fs_index(fs) + 1)
    c["lastnz_first"] = dict(lastnz=coded_lines(fs, ms, hr) // 2)
    c["order8"] = dict(tns0=1, head=(255, 128))        # low at the top of the interval: the order symbol is the last one, 8
    c["gg255"] = dict(gg=255); c["gg0"] = dict(gg=0)
    if (fs, ms, size) == (48000, 10.0, 20):
        # The TNS reader collision with a valid range-decoder state.  Below 480 bits the order model's last symbol starts at 839 / 1024: a head of
        # (0xFFFFFF >> 10) * 839 = 0xD1BCB9 decodes order 8 and leaves low = 0, and every zero byte behind it decodes coefficient symbol 0 at ten bits
        # apiece, so the forward reader walks into the side information (the backward reader stands at byte 11) before the eighth coefficient.  About a
        # third of these are frames that ONLY this check refuses: a parser without it decodes them to the end and finds nres >= 0.
        for j in (8, 10, 12, 13):
            for tns1 in (0, 1):
                c["tns_reader_%d_%d" % (j, tns1)] = dict(head=(0xD1, 0xBC, 0xB9) + (0,) * (j - 3), bw=4, lastnz=tns1, tns0=1, tns1=tns1, ltpf=0)
    return c


# ---- pools ---------------------------------------------------------------------------------------------------------------------------------------------
Attr = collections.namedtuple("Attr", "order ltpf gg")
DRAWS = 6000
DRAWS_AT = {(96000, 2.5, 1, 62): 12000}             # nres < 0 turns up about once in 1400 payloads there
DRAWS_TINY = 80000                                 # 48 kHz / 10 ms / 20 bytes: the TNS reader collision turns up about once in 5000 payloads
PER_CRAFT = 3
ACC_CAP = 1000


def _verdict(dec, tr, p):
    rc, _ = dec.decode(p)
    assert rc in (0, 2), rc
    return dec.last_reject(), Attr(max(tr[0].tns_order[0], tr[0].tns_order[1]), tr[0].ltpf[1], tr[0].gg_idx) if rc == 0 else None


@functools.lru_cache(maxsize=None)
def pool(fs, ms, hr, size):
    """-> (accepted [(payload, Attr, origin)], refused {reason: [(payload, origin)]}): the crafted ones first, then the drawn ones in the order drawn"""
    dec = OracleDecoder(fs, 1, ms, hr, portable_math=True)
    tr = dec.enable_trace()
    rng = np.random.RandomState((fs // 100 * 7919 + int(ms * 10) * 104729 + hr * 15485863 + size * 32452843) & 0x7FFFFFFF)
    acc, rej = [], collections.OrderedDict((r, []) for r in REASONS)
    tiny = fs == 48000 and ms == 10.0 and size == 20
    for _ in range((DRAWS_TINY if tiny else DRAWS_AT.get((fs, ms, hr, size), DRAWS)) // 2000):
        for p in rng.randint(0, 256, size=(2000, size)).astype(np.uint8):
            why, a = _verdict(dec, tr, p)
            if why == 0 and len(acc) < ACC_CAP:
                acc.append((p, a, "drawn"))
            elif why and len(rej[why]) < 12:
                rej[why].append((p, "drawn"))
        if tiny and len(rej[REJ_TNS_READER]) >= 6 and len(acc) >= 300:
            break
    assert len(acc) >= 100, (fs, ms, hr, size, len(acc))
    c_acc, c_rej = [], collections.OrderedDict((r, []) for r in REASONS)
    for i, (name, ed) in enumerate(crafts(fs, ms, hr, size).items()):
        for j in range(PER_CRAFT):
            p = edit(acc[(i * PER_CRAFT + j) % len(acc)][0], fs, ms, hr, **ed)
            why, a = _verdict(dec, tr, p)
            if why == 0:
                c_acc.append((p, a, name))
            else:
                c_rej[why].append((p, name))
    # a genuine spectrum under a hostile gain: full-scale noise as the oracle encoder codes it, ten times (28 steps) louder - far into the 16-bit clamp
    enc = Oracle(fs, 1, ms, hr, size * 8 * 1000 * 10 // int(ms * 10), portable_math=True)
    assert enc.nbytes == size
    for x in rng.randint(-32768, 32768, size=(3 + PER_CRAFT, 1, frame_len(fs, ms))).astype(np.int16):
        p = enc.encode(x)
        p = edit(p, fs, ms, hr, gg=min(255, get_bits(p, *side_fields(p, fs, ms, hr)["gg"]) + 28))
        why, a = _verdict(dec, tr, p)
        assert why == 0
        c_acc.append((p, a, "loud"))
    c_acc = c_acc[:-3 - PER_CRAFT] + c_acc[-PER_CRAFT:]                     # (not the encoder's first frames)
    return c_acc + acc, collections.OrderedDict((r, c_rej[r] + rej[r]) for r in REASONS)


def _accepted_sequence(acc, ms, n):
    """n accepted payloads: first the crafted ones, then those with a TNS order of at least maxlag - 1, the LTPF switched on, a global gain of at least 200 and of at most 20, four
    of a kind in turn, then whatever is left in pool order"""
    hi = max_lag(ms) - 1
    cats = [[x for x in acc if x[1].order >= hi], [x for x in acc if x[1].ltpf == 1], [x for x in acc if x[1].gg >= 200], [x for x in acc if x[1].gg <= 20]]
    quota = [26, 12, 7, 7]
    out, used = [], set()

    def add(x):
        if id(x) not in used and len(out) < n:
            used.add(id(x)); out.append(x)
    for x in acc:
        if x[2] != "drawn":
            add(x)
    for k in range(max(quota)):
        for c, q in zip(cats, quota):
            if k < q and k < len(c):
                add(c[k])
    for x in acc:
        add(x)
    assert len(out) == n
    return out


class _Turns:
    """the refused payloads of one size, dealt out so that the reason changes with every frame.  `rare`: reasons that take every other turn; `first`: the
    order of the others"""
    def __init__(self, rej, rare=(), first=REASONS, clock=None):
        self.rej = rej
        self.clock = clock if clock is not None else [0]             # (the two channel sizes of a stereo geometry share it)
        self.common = [r for r in first if rej[r] and r not in rare]
        self.rare = [r for r in REASONS if rej[r] and r in rare]
        self.used = collections.Counter()

    def next(self):
        n = self.clock[0]
        if self.rare and n % 2 == 0:
            r = self.rare[(n // 2) % len(self.rare)]
        else:
            r = self.common[(n // 2 if self.rare else n) % len(self.common)]
        self.clock[0] += 1
        p = self.rej[r][self.used[r] % len(self.rej[r])][0]
        self.used[r] += 1
        return p

    def filler(self):
        return self.rej[(self.common + self.rare)[0]][0][0]


def reachable(fs, ms, hr, size):
    return {r for r, v in pool(fs, ms, hr, size)[1].items() if v}


def _kinds(pattern, where):
    """kind [T] of a pattern, and for stereo the channel(s) of each refused frame"""
    k = np.full(T, G, np.int64)
    t = np.arange(T)
    if pattern == "r_first":
        k[t % 3 == 0] = R
    elif pattern == "r_behind_g":
        k[t % 3 == 2] = R
    elif pattern in ("r_behind_h", "h_r1"):
        k[:] = H; k[t % 3 == 2] = R
    elif pattern == "all_h":
        k[:] = H
    elif pattern == "alternating":
        k[:] = np.array([G, R, H, R])[t % 4]
    elif pattern == "burst":
        k[BURST[0]:BURST[0] + len(BURST[1])] = BURST[1]; k[BURST[0] + len(BURST[1])] = H
    elif pattern == "size_change":
        k[[4, 9, CUT, 18]] = R
    else:
        raise KeyError(pattern)
    n = 0
    ch = [""] * T
    for i in range(T):
        if k[i] == R and where:
            ch[i] = where[n % len(where)]; n += 1
    return k, ch


def patterns(geom):
    n = len(GEOMS[geom][4])
    return PATTERNS[:n]


def stream_sizes(geom):
    """[B, T] the size every stream-frame is coded at (kept for flagged and empty frames: sizes of streams() is 0 where the frame is empty)"""
    out = np.zeros((len(GEOMS[geom][4]), T), np.int64)
    for b, z in enumerate(GEOMS[geom][4]):
        out[b] = z if isinstance(z, int) else np.where(np.arange(T) < CUT, z[0], z[1])
    return out


def _genuine(fs, ms, hr, sizes_t, seed):
    """[T] payloads of one channel: the oracle encoder on synth_pcm, the bitrate following sizes_t"""
    pcm = synth_pcm(1, T, frame_len(fs, ms), fs, seed=seed)[0]
    enc, out = None, []
    for t in range(T):
        br = int(sizes_t[t]) * 8 * 1000 * 10 // int(ms * 10)
        if enc is None:
            enc = Oracle(fs, 1, ms, hr, br, portable_math=True)
        elif sizes_t[t] != sizes_t[t - 1]:
            assert enc.set_bitrate(br) == 0
        assert enc.nbytes == sizes_t[t], (enc.nbytes, sizes_t[t])
        out.append(enc.encode(pcm[t][None, :]))
    return out


@functools.lru_cache(maxsize=None)
def streams(geom):
    """-> frames uint8 [B, T, stride] (zero behind a payload), sizes [B, T] (int32; 0: an empty frame), bfi uint8 [B, T], kind uint8 [B, T], reason uint8 [B * channels, T]
    (what the oracle gives decoding them; 0 for decoded, flagged and empty frames and for a second channel behind a refused first one).  Read-only."""
    fs, ms, hr, ch, zs = GEOMS[geom]
    full = stream_sizes(geom)
    B = len(zs)
    frames = np.zeros((B, T, int(full.max())), np.uint8)
    kind = np.zeros((B, T), np.int64)
    every = sorted({z for row in full for tot in set(row.tolist()) for z in channel_sizes(tot, ch)})
    only = {z: set(REASONS) for z in every}                               # reasons no other size of the geometry reaches
    for z in every:
        for y in every:
            if y != z:
                only[z] -= reachable(fs, ms, hr, y)
    first = sorted(REASONS, key=lambda r: (sum(r in reachable(fs, ms, hr, z) for z in every), r))     # what the fewest sizes reach leads every size's turns
    clock = [0] if ch == 2 else None
    turns = {z: _Turns(pool(fs, ms, hr, z)[1], only[z] if len(every) > 1 and ch == 1 else (), first, clock) for z in every}
    accepted = {z: iter(_accepted_sequence(pool(fs, ms, hr, z)[0], ms, min(len(pool(fs, ms, hr, z)[0]), 120))) for z in every}
    for b, pat in enumerate(patterns(geom)):
        kind[b], where = _kinds(pat, STEREO_WHERE.get(pat, "") if ch == 2 else "")
        zt = [[channel_sizes(int(x), ch)[c] for x in full[b]] for c in range(ch)]
        assert ch == 1 or all(len(set(z)) == 1 for z in zt)               # (a stereo stream keeps its size)
        gen = [_genuine(fs, ms, hr, zt[c], seed=1000 + 16 * b + c) for c in range(ch)]
        for t in range(T):
            at = 0
            for c in range(ch):
                k, z = kind[b, t], zt[c][t]
                if k == G:
                    p = gen[c][t]
                elif k == R and (ch == 1 or where[t] in ("b", str(c))):
                    p = turns[z].next()
                elif k in (FLAG, EMPTY):                                    # the slot of a flagged or empty frame is never read
                    p = turns[z].filler()
                else:
                    p = next(accepted[z])[0]
                frames[b, t, at:at + z] = p
                at += z
    bfi = (kind == FLAG).astype(np.uint8)
    sizes = np.where(kind == EMPTY, 0, full)
    reason = decode(geom, frames, sizes, bfi)["reason"]                    # (the verdict on a payload depends on nothing but its size)
    out = (frames, sizes.astype(np.int32), bfi, kind.astype(np.uint8), reason.astype(np.uint8))
    for a in out:
        a.flags.writeable = False
    return out


def as_flags(sizes, bfi, full):
    """the same losses, every one given through bfi: (sizes without a 0, flags)"""
    return np.where(sizes == 0, full, sizes), (bfi | (sizes == 0)).astype(np.uint8)


def as_empty(sizes, bfi):
    """the same losses, every one given as size 0: (sizes, no flags)"""
    return np.where(bfi == 1, 0, sizes), np.zeros_like(bfi)


def decode(geom, frames, sizes, bfi, portable_math=True, bps=16, dec_cls=None, rows=None):
    """The streams (or the streams `rows`) through one decoder each, a frame at a time with its own size -> dict: pcm [B, T, channels, N], status [B, T]
    (1 = concealed); with the oracle also reason [B * channels, T], order / ltpf / gg [B * channels, T] (-1 where not decoded) and peak [B, T], the largest
    |x_out| of the frame over its channels.  dec_cls: RefDecoder - an empty frame is then given as flagged, which is the same thing (R/lc3.c:277-282)."""
    fs, ms, hr, ch, _ = GEOMS[geom]
    rows = list(range(frames.shape[0])) if rows is None else list(rows)
    B, n_t, N = len(rows), frames.shape[1], frame_len(fs, ms)
    o = dict(pcm=np.zeros((B, n_t, ch, N), np.int16 if bps == 16 else np.int32), status=np.zeros((B, n_t), np.uint8))
    if dec_cls is None:
        o.update(reason=np.zeros((B * ch, n_t), np.int64), peak=np.zeros((B, n_t)))
        o.update({k: np.full((B * ch, n_t), -1, np.int64) for k in ("order", "ltpf", "gg")})
    for i, b in enumerate(rows):
        d = dec_cls(fs, ch, ms, hr) if dec_cls else OracleDecoder(fs, ch, ms, hr, portable_math=portable_math)
        tr = None if dec_cls else d.enable_trace()
        for t in range(n_t):
            nb, flag = int(sizes[b, t]), int(bfi[b, t])
            if dec_cls:
                rc, x = d.decode(frames[b, t, :max(nb, 1)], 1 if nb == 0 else flag, bps)
            else:
                rc, x = d.decode(frames[b, t, :max(nb, 1)], flag, bps, num_bytes=nb)
            assert rc in (0, 2), (geom, b, t, rc)
            o["pcm"][i, t], o["status"][i, t] = x, rc == 2
            if tr is not None:
                for c in range(ch):
                    o["reason"][i * ch + c, t] = d.last_reject(c)
                    if tr[c].bfi == 0:
                        o["order"][i * ch + c, t] = max(tr[c].tns_order[0], tr[c].tns_order[1])
                        o["ltpf"][i * ch + c, t], o["gg"][i * ch + c, t] = tr[c].ltpf[1], tr[c].gg_idx
                o["peak"][i, t] = max(float(np.abs(np.ctypeslib.as_array(tr[c].x_out)[:N]).max()) for c in range(ch))
    return o


def ltpf_enabled(fs, ms, hr, nbytes):
    """whether a channel of nbytes has the LTPF at all (R/setup_dec_lc3.c:188-299)"""
    bits = nbytes * 8
    bits = int(bits * 4.0 * (1.0 - 0.4)) if ms == 2.5 else bits * 2 - 160 if ms == 5.0 else bits
    return hr == 0 and bits < 640 + 80 * (fs_index(fs) - 1)


@functools.lru_cache(maxsize=None)
def _peaks(geom):
    frames, sizes, bfi, kind, reason = streams(geom)
    return decode(geom, frames, sizes, bfi)["peak"].max(axis=1)


def depth_streams(geom, bps):
    """the streams whose 24- or 32-bit output is defined: max |x_out| 2^(bps - 16) < 2^31 over the whole stream (the reference casts the rounded product to
    int32_t); tests/test_hostile_frames_cpu.py asserts the bound on them"""
    return [b for b, p in enumerate(_peaks(geom)) if p * 2.0 ** (bps - 16) < 2.0 ** 31]


def lost_equivalent(geom):
    """(streams for which decoding a refused frame equals decoding it flagged, stereo streams for which it must not): every mono stream but the one that
    changes its size at a refused frame; the stereo streams whose refusals are all in channel 0, and those with one in channel 1"""
    pats = patterns(geom)
    if GEOMS[geom][3] == 1:
        return [i for i, p in enumerate(pats) if p != "size_change"], []
    return [i for i, p in enumerate(pats) if "1" not in STEREO_WHERE.get(p, "")], [i for i, p in enumerate(pats) if "1" in STEREO_WHERE.get(p, "")]


@functools.lru_cache(maxsize=None)
def tail(geom, n=4):
    """n further genuine frames per stream at the size of its last frame -> uint8 [B, n, stride]: what the GPU tests decode behind the streams to see the state
    they left"""
    fs, ms, hr, ch, zs = GEOMS[geom]
    full = stream_sizes(geom)
    out = np.zeros((len(zs), n, int(full.max())), np.uint8)
    for b in range(len(zs)):
        at = 0
        for c, z in enumerate(channel_sizes(int(full[b, -1]), ch)):
            out[b, :, at:at + z] = np.stack(_genuine(fs, ms, hr, [z] * T, seed=2000 + 16 * b + c)[T - n:])
            at += z
    out.flags.writeable = False
    return out
