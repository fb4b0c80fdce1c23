"""Every pair of options of one call (test helper beside launch_census.py, TEST INFRASTRUCTURE ONLY).

The host runtime (audio_codec_amd/csrc/lc3_runtime.hip: enc_launch, enc_one_wave, launch_resample, dec_parse, dec_chain) picks its kernels from the product of a
call's options; tests/launch_census.py runs every entry point in one scenario each.  Here: the options as factors (ENC_FACTORS, DEC_FACTORS), what the library
refuses as one list of clauses per side (ENC_CLAUSES, DEC_CLAUSES - every one a check of lc3_host.c or a `return 1` of lc3_runtime.hip, or the plain fact that a
call has no such argument), a covering-array generator (generate) and its output as literal tables (ENC_ROWS, DEC_ROWS): full rows in which every pair of levels
of two different factors that some valid call can have occurs at least once.  RESAMPLE_ROWS: the one launch decision that takes four factors at once, in full.  tests/test_option_pairs_cpu.py holds the tables to the generator, the clauses to
the host code and the coverage to a brute-force count; tests/test_gpu_option_pairs.py runs every row through the census engines against the CPU oracle.

A row is a tuple of levels in the order of the side's factors; a partial row is a dict {factor: level}.  A clause speaks of two factors, so valid() of a partial
row looks at the clauses whose two factors the row has; a pair is valid if some full valid row contains it (completes).

Regenerate the tables: python tests/option_pairs.py"""
import collections

import launch_census as lc

GEOMS = {n: getattr(lc, n) for n in ("G48", "G48S", "G48_5S", "G48_25S", "G32S", "G16S", "G48HR", "G96S", "G96_5S", "G96_25S", "G44S", "G48LS")}
HR = tuple(n for n, g in GEOMS.items() if g[2])                             # high resolution: no per-frame bandwidths
FORMS = (16, 24, 32, "f32", "s16be", "s24_3le", "s24_3be", "ulaw", "alaw")
ELEM_BYTES = {16: 2, 24: 4, 32: 4, "f32": 4, "s16be": 2, "s24_3le": 3, "s24_3be": 3, "ulaw": 1, "alaw": 1}
LAYOUTS = ("default", "interleaved", "channel_major")
# both paths, both hand-overs between them, the five-wave writer's threshold (48 frames) and the two sides of LC3D_FUSED_MAX_T (8) ...
ENC_CALLS = ((2, 2), (12, 12), (2, 12), (12, 2), (48, 9), (9, 8))
# ... and under the input-ready promise of LC3D_FUSED_MAX_T_READY (5)
ENC_CALLS_READY = {(2, 2): (2, 2), (12, 12): (12, 12), (2, 12): (2, 12), (12, 2): (12, 2), (48, 9): (48, 6), (9, 8): (6, 5)}
DEC_CALLS = ((2, 12), (12, 2), (12, 12), (1, 9), (48, 3))

ENC_FACTORS = (
    ("geom", tuple(n for n in GEOMS if n != "G48LS")),                      # G48LS is there for the decoder's _g parsers
    ("calls", ENC_CALLS),
    ("how", ("host", "device", "hostwords", "rates", "packed")),
    ("words", ("", "r", "b", "rb")),
    ("form", FORMS),
    ("layout", LAYOUTS),
    ("placed", (0, 1)),
    ("ragged", (0, 1)),
    ("ready", (0, 1)),
    ("reset", (0, 1)),                                                      # stream 1 between the calls
    ("pad", (0, 1, 3)),                                                     # elements of the form's size the PCM pointer lies behind a 256-byte boundary
    ("order", (0, 1)),                                                      # api.PACK_STREAM_MAJOR, api.PACK_FRAME_MAJOR
)
DEC_FACTORS = (
    ("geom", tuple(GEOMS)),
    ("calls", DEC_CALLS),
    ("how", ("host", "hostsizes", "device", "devhostsizes", "sizes", "packed")),
    ("out", FORMS),
    ("layout", LAYOUTS),
    ("placed", (0, 1)),
    ("ragged", (0, 1)),
    ("ready", (0, 1)),
    ("reset", (0, 1)),
    ("pad", (0, 1, 3)),                                                     # on the PCM output pointer
)

# kind "refusal": the library returns an error for the pair, and the tests make that call; kind "shape": the call named by `how` has no such argument, so there
# is no call to make
Clause = collections.namedtuple("Clause", "name kind fa fb hits where")
_HOST_PCM = ("host", "hostsizes")
ENC_CLAUSES = (
    # lc3_host.c batch_encode, batch_encode_bitrates, batch_encode_bandwidths: `if (b->ragged) return LC3_ERROR`; lc3_runtime.hip lc3hip_encode: `if (c->counts) return 1`
    Clause("ragged_call", "refusal", "how", "ragged", lambda how, ragged: ragged and how in ("host", "device", "hostwords"),
           "lc3_host.c batch_encode / batch_encode_bitrates / batch_encode_bandwidths: b->ragged; lc3_runtime.hip lc3hip_encode: c->counts"),
    # lc3_host.c lc3plus_enc_batch_encode_rates_device: `(!bitrates && !bandwidths)` is LC3_NULL_ERROR, with or without frame counts
    Clause("rates_words", "refusal", "how", "words", lambda how, words: how == "rates" and words == "",
           "lc3_host.c lc3plus_enc_batch_encode_rates_device: !bitrates && !bandwidths"),
    # lc3plus_enc_batch_encode has no bitrates or bandwidths argument: the device-pointer call with host words is `hostwords` ...
    Clause("device_words", "shape", "how", "words", lambda how, words: how == "device" and words != "", "lc3plus_enc_batch_encode: no words argument"),
    # ... and lc3plus_enc_batch_encode_bitrates / _bandwidths without their array are LC3_NULL_ERROR: the call without words is `device`
    Clause("hostwords_words", "shape", "how", "words", lambda how, words: how == "hostwords" and words == "",
           "lc3_host.c batch_encode_bitrates / batch_encode_bandwidths: the call without its words is lc3plus_enc_batch_encode"),
    # lc3_host.c placed_refuses: `placed && !pcm_on_device`; lc3_runtime.hip lc3hip_encode: `if (c->plo && (!pcm_on_device || trace_host)) return 1`
    Clause("host_placed", "refusal", "how", "placed", lambda how, placed: placed and how == "host", "lc3_host.c placed_refuses: !pcm_on_device; lc3_runtime.hip lc3hip_encode: c->plo"),
    # a host array has no device pointer to move, and the promise speaks of device-pointer calls (include/lc3plus_batch.h: lc3plus_enc_batch_set_input_ready)
    Clause("host_pad", "shape", "how", "pad", lambda how, pad: pad and how == "host", "a host array: no device pointer"),
    Clause("host_ready", "shape", "how", "ready", lambda how, ready: ready and how == "host", "lc3plus_enc_batch_set_input_ready: device-pointer calls"),
    # lc3_host.c placed_refuses: `format & LC3D_PCM_CHANNEL_MAJOR`; lc3plus_plan_placed refuses the layout; lc3_runtime.hip enc_launch: `if (q.placed && (... (bitdepth & LC3D_PCM_CHANNEL_MAJOR))) return 1`
    Clause("placed_channel_major", "refusal", "placed", "layout", lambda placed, layout: placed and layout == "channel_major",
           "lc3_host.c placed_refuses, lc3plus_plan_placed: LC3D_PCM_CHANNEL_MAJOR; lc3_runtime.hip enc_launch: q.placed"),
    # lc3_host.c batch_encode_bandwidths, lc3plus_enc_batch_encode_rates_device, lc3plus_enc_batch_encode_packed: LC3_HRMODE_BW_ERROR; lc3_runtime.hip lc3hip_encode
    # `if (bw_host && c->big) return 1`, lc3hip_encode_rates_device `bws_dev && c->big`, enc_one_wave `if (c->big && q->dbw) return 1`
    Clause("bandwidth_hr", "refusal", "geom", "words", lambda geom, words: "b" in words and geom in HR,
           "lc3_host.c batch_encode_bandwidths, lc3plus_enc_batch_encode_rates_device, lc3plus_enc_batch_encode_packed: g.hrmode; lc3_runtime.hip enc_one_wave: c->big && q->dbw"),
    # only lc3plus_enc_batch_encode_packed has an order
    Clause("order_packed", "shape", "how", "order", lambda how, order: order and how != "packed", "lc3plus_enc_batch_encode_packed alone takes an order"),
)
DEC_CLAUSES = (
    # lc3_host.c dec_batch_decode, lc3plus_dec_batch_decode_sizes: `if (b->ragged) return LC3_ERROR`; lc3_runtime.hip dec_decode: `if (q->cnt && !q->nb_dev) return 1`
    Clause("ragged_call", "refusal", "how", "ragged", lambda how, ragged: ragged and how in ("host", "hostsizes", "device", "devhostsizes"),
           "lc3_host.c dec_batch_decode, lc3plus_dec_batch_decode_sizes: b->ragged; lc3_runtime.hip dec_decode: q->cnt && !q->nb_dev"),
    # lc3_host.c placed_refuses: `placed && !pcm_on_device`; lc3_runtime.hip dec_decode: `if (c->plo && (!q->pcm_on_device || ...)) return 1`
    Clause("host_placed", "refusal", "how", "placed", lambda how, placed: placed and how in _HOST_PCM, "lc3_host.c placed_refuses: !pcm_on_device; lc3_runtime.hip dec_decode: c->plo"),
    Clause("host_pad", "shape", "how", "pad", lambda how, pad: pad and how in _HOST_PCM, "a host array: no device pointer"),
    Clause("host_ready", "shape", "how", "ready", lambda how, ready: ready and how in _HOST_PCM, "lc3plus_dec_batch_set_input_ready: device-pointer calls"),
    # lc3_host.c placed_refuses: `format & LC3D_PCM_CHANNEL_MAJOR`; lc3_runtime.hip dec_decode: `if (c->plo && (... (q->bps & LC3D_PCM_CHANNEL_MAJOR))) return 1`
    Clause("placed_channel_major", "refusal", "placed", "layout", lambda placed, layout: placed and layout == "channel_major",
           "lc3_host.c placed_refuses, lc3plus_plan_placed: LC3D_PCM_CHANNEL_MAJOR; lc3_runtime.hip dec_decode: c->plo"),
)
SIDES = {"enc": (ENC_FACTORS, ENC_CLAUSES), "dec": (DEC_FACTORS, DEC_CLAUSES)}
# every refusal above is made by lc3_host.c before the runtime is asked, so the build of lc3_host.c over tools/stub_shim.c reaches all of them without a GPU;
# the runtime's own `return 1` behind each is what tests/test_gpu_option_pairs.py would have to reach for a clause listed here
GPU_ONLY_CLAUSES = {"enc": (), "dec": ()}


def violations(side, row):
    """the names of the clauses a partial or full row (dict) breaks"""
    return [c.name for c in SIDES[side][1] if c.fa in row and c.fb in row and c.hits(row[c.fa], row[c.fb])]


def valid(side, row):
    return not violations(side, row)


def as_dict(side, row):
    return dict(zip((f for f, _ in SIDES[side][0]), row))


def completes(side, partial, ok=valid):
    """a full row (dict) that contains the partial one and that ok() accepts, or None: depth first over the factors left, levels in table order"""
    factors = [(f, lv) for f, lv in SIDES[side][0] if f not in partial]
    row = dict(partial)
    if not ok(side, row):
        return None

    def go(i):
        if i == len(factors):
            return dict(row)
        f, levels = factors[i]
        for v in levels:
            row[f] = v
            if ok(side, row):
                r = go(i + 1)
                if r:
                    return r
        row.pop(f, None)
        return None
    return go(0)


def all_pairs(side):
    """every pair of levels of two different factors as (i, a, j, b): factor numbers i < j, level numbers a, b"""
    fs = SIDES[side][0]
    return [(i, a, j, b) for i in range(len(fs)) for j in range(i + 1, len(fs)) for a in range(len(fs[i][1])) for b in range(len(fs[j][1]))]


def pair_dict(side, p):
    fs = SIDES[side][0]
    return {fs[p[0]][0]: fs[p[0]][1][p[1]], fs[p[2]][0]: fs[p[2]][1][p[3]]}


def valid_pairs(side):
    return {p for p in all_pairs(side) if completes(side, pair_dict(side, p))}


def row_pairs(side, row):
    """the pairs a full row (tuple of levels) contains"""
    fs = SIDES[side][0]
    ix = [fs[i][1].index(v) for i, v in enumerate(row)]
    return {(i, ix[i], j, ix[j]) for i in range(len(ix)) for j in range(i + 1, len(ix))}


class _Lcg:
    """the generator's own random numbers: the same on every Python"""
    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def below(self, n):
        self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
        return (self.x >> 8) % n

    def shuffled(self, seq):
        seq = list(seq)
        for i in range(len(seq) - 1, 0, -1):
            j = self.below(i + 1)
            seq[i], seq[j] = seq[j], seq[i]
        return seq


def generate(side, seed=20, tries=12):
    """Greedy covering array.  Until every valid pair is covered: `tries` candidate rows, each grown from an uncovered pair of the two factors with the most
    levels that still have one (the rows cannot be fewer than the product of the two largest factors, so those pairs set the pace), the other factors in a
    random order, each at the level that covers the most uncovered pairs with the levels chosen so far among those that keep the row completable; the candidate
    that covers most is kept.  Returns the rows as tuples of levels."""
    fs = SIDES[side][0]
    rng = _Lcg(seed)
    good = valid_pairs(side)
    left = set(good)
    rows = []

    def key(i, a, j, b):
        return (i, a, j, b) if i < j else (j, b, i, a)
    while left:
        size = max(len(fs[p[0]][1]) * len(fs[p[2]][1]) for p in left)
        seeds = sorted(p for p in left if len(fs[p[0]][1]) * len(fs[p[2]][1]) == size)
        best = None
        for _ in range(tries):
            p = seeds[rng.below(len(seeds))]
            ix = {p[0]: p[1], p[2]: p[3]}
            for i in rng.shuffled(k for k in range(len(fs)) if k not in ix):
                cands = []
                for a in rng.shuffled(range(len(fs[i][1]))):
                    if all(key(i, a, j, b) in good for j, b in ix.items()):
                        cands.append((sum(key(i, a, j, b) in left for j, b in ix.items()), a))
                cands.sort(key=lambda c: -c[0])                              # stable: ties stay in the shuffled order
                for _, a in cands:
                    ix[i] = a
                    if completes(side, {fs[k][0]: fs[k][1][v] for k, v in ix.items()}):
                        break
                    del ix[i]
                assert i in ix, "a completable row has a level for every factor"
            row = tuple(fs[k][1][ix[k]] for k in range(len(fs)))
            gain = len(row_pairs(side, row) & left)
            if best is None or gain > best[0]:
                best = (gain, row)
        rows.append(best[1])
        left -= row_pairs(side, best[1])
    return rows


def excluded_by_clause(side):
    """{clause name: [excluded pairs]}: every pair no valid row contains under the one clause that names its two levels; a pair no clause names (excluded only
    through other factors) goes under None"""
    out = collections.defaultdict(list)
    good = valid_pairs(side)
    for p in all_pairs(side):
        if p not in good:
            v = violations(side, pair_dict(side, p))
            out[v[0] if len(v) == 1 else None if not v else tuple(v)].append(p)
    return dict(out)


def only_breaks(side, pair, clause):
    """a full row (dict) that contains the excluded pair and breaks `clause` alone: the call the refusal tests make"""
    return completes(side, pair_dict(side, pair), ok=lambda s, r: set(violations(s, r)) <= {clause})


def scenario(side, n, row, prefix=None):
    """the census engines' scenario (launch_census.run_encoder / run_decoder) of a full row"""
    r = as_dict(side, row) if not isinstance(row, dict) else row
    form = r["form" if side == "enc" else "out"]
    sc = dict(kind=side, name="%s%03d" % (prefix or side, n), geom=GEOMS[r["geom"]], claims=(), how=r["how"], layout=None if r["layout"] == "default" else r["layout"],
              placed=bool(r["placed"]), ragged=bool(r["ragged"]), ready=bool(r["ready"]), reset=(1,) if r["reset"] else (), pad=r["pad"] * ELEM_BYTES[form])
    if side == "enc":
        sc.update(calls=ENC_CALLS_READY[r["calls"]] if r["ready"] else r["calls"], words=r["words"], form=form, order=r["order"])
    else:
        sc.update(calls=r["calls"], out=form)
    return sc


# counts the CPU test pins (test_option_pairs_cpu.py recomputes them): valid pairs, excluded pairs per clause
COUNTS = {
    "enc": dict(pairs=1142, valid=1117, excluded=dict(ragged_call=3, rates_words=1, device_words=3, hostwords_words=1, host_placed=1, host_pad=2, host_ready=1, placed_channel_major=1, bandwidth_hr=8, order_packed=4)),
    "dec": dict(pairs=898, valid=885, excluded=dict(ragged_call=4, host_placed=2, host_pad=4, host_ready=2, placed_channel_major=1)),
}

# ---------------------------------------------------------------------------------------------------------------------------------------------------
# generate("enc") and generate("dec"), committed: tests/test_option_pairs_cpu.py compares
# ---------------------------------------------------------------------------------------------------------------------------------------------------
ENC_ROWS = (
    ('G48_5S', (2, 12), 'packed', '', 's24_3le', 'default', 1, 0, 1, 1, 1, 1),
    ('G48', (12, 2), 'packed', 'r', 'ulaw', 'interleaved', 0, 1, 0, 0, 0, 0),
    ('G48S', (48, 9), 'hostwords', 'b', 's24_3be', 'interleaved', 1, 0, 1, 0, 3, 0),
    ('G48S', (9, 8), 'rates', 'rb', 32, 'channel_major', 0, 1, 0, 1, 1, 0),
    ('G44S', (2, 2), 'device', '', 'alaw', 'default', 0, 0, 0, 0, 3, 0),
    ('G96_25S', (12, 12), 'packed', 'r', 24, 'channel_major', 0, 0, 1, 0, 3, 1),
    ('G16S', (2, 2), 'packed', 'b', 16, 'interleaved', 1, 1, 0, 1, 0, 1),
    ('G32S', (2, 12), 'host', 'rb', 24, 'interleaved', 0, 0, 0, 0, 0, 0),
    ('G96_25S', (9, 8), 'hostwords', 'r', 's16be', 'default', 1, 0, 0, 1, 0, 0),
    ('G48', (48, 9), 'packed', 'rb', 'alaw', 'default', 1, 1, 1, 1, 3, 1),
    ('G32S', (12, 2), 'rates', 'b', 16, 'default', 1, 0, 1, 1, 1, 0),
    ('G48HR', (48, 9), 'rates', 'r', 's24_3le', 'channel_major', 0, 1, 0, 0, 0, 0),
    ('G16S', (12, 12), 'device', '', 'f32', 'channel_major', 0, 0, 1, 0, 0, 0),
    ('G96S', (9, 8), 'packed', '', 's16be', 'interleaved', 0, 1, 1, 0, 3, 1),
    ('G96_5S', (12, 12), 'packed', '', 's24_3be', 'default', 1, 1, 0, 1, 0, 1),
    ('G48_25S', (2, 12), 'hostwords', 'b', 'alaw', 'channel_major', 0, 0, 1, 0, 1, 0),
    ('G48HR', (2, 2), 'device', '', 32, 'interleaved', 1, 0, 1, 1, 1, 0),
    ('G48_25S', (2, 2), 'rates', 'rb', 'ulaw', 'default', 1, 0, 0, 1, 3, 0),
    ('G44S', (12, 12), 'rates', 'b', 24, 'interleaved', 1, 1, 1, 1, 1, 0),
    ('G32S', (2, 12), 'packed', 'r', 32, 'channel_major', 0, 1, 1, 0, 3, 1),
    ('G48S', (2, 2), 'host', 'r', 'f32', 'default', 0, 0, 0, 1, 0, 0),
    ('G48_5S', (12, 2), 'rates', 'rb', 's24_3be', 'channel_major', 0, 1, 0, 0, 3, 0),
    ('G96_5S', (2, 12), 'rates', 'r', 's16be', 'channel_major', 0, 0, 1, 0, 1, 0),
    ('G96_5S', (12, 2), 'packed', '', 'f32', 'interleaved', 1, 1, 1, 1, 3, 1),
    ('G96S', (2, 2), 'hostwords', 'r', 's24_3be', 'channel_major', 0, 0, 0, 1, 1, 0),
    ('G96_25S', (48, 9), 'packed', '', 'ulaw', 'interleaved', 1, 1, 1, 1, 1, 1),
    ('G48', (12, 12), 'host', 'b', 32, 'channel_major', 0, 0, 0, 1, 0, 0),
    ('G96S', (48, 9), 'device', '', 24, 'default', 1, 0, 0, 0, 0, 0),
    ('G48_25S', (12, 12), 'packed', 'r', 16, 'channel_major', 0, 1, 0, 0, 3, 1),
    ('G48_5S', (9, 8), 'hostwords', 'b', 'f32', 'interleaved', 0, 0, 0, 0, 0, 0),
    ('G44S', (12, 12), 'hostwords', 'rb', 's24_3le', 'channel_major', 0, 0, 0, 0, 3, 0),
    ('G48_5S', (12, 12), 'host', 'r', 'alaw', 'interleaved', 0, 0, 0, 1, 0, 0),
    ('G48_25S', (12, 2), 'device', '', 's16be', 'interleaved', 0, 0, 0, 0, 0, 0),
    ('G16S', (48, 9), 'rates', 'rb', 's16be', 'default', 1, 1, 1, 1, 1, 0),
    ('G44S', (2, 12), 'packed', 'r', 'ulaw', 'channel_major', 0, 1, 0, 0, 0, 1),
    ('G48_25S', (9, 8), 'host', 'b', 's24_3le', 'interleaved', 0, 0, 0, 1, 0, 0),
    ('G48', (2, 12), 'rates', 'rb', 'f32', 'interleaved', 0, 0, 1, 0, 1, 0),
    ('G48HR', (12, 12), 'packed', 'r', 's16be', 'default', 0, 0, 0, 1, 3, 1),
    ('G44S', (48, 9), 'host', '', 16, 'channel_major', 0, 0, 0, 1, 0, 0),
    ('G96S', (12, 2), 'hostwords', 'r', 32, 'default', 0, 0, 0, 1, 0, 0),
    ('G48S', (2, 12), 'packed', '', 16, 'default', 0, 1, 0, 0, 1, 1),
    ('G32S', (9, 8), 'device', '', 's24_3be', 'interleaved', 0, 0, 0, 1, 0, 0),
    ('G48', (2, 2), 'device', '', 's24_3le', 'channel_major', 0, 0, 0, 1, 0, 0),
    ('G48', (9, 8), 'hostwords', 'rb', 16, 'channel_major', 0, 0, 1, 0, 3, 0),
    ('G16S', (9, 8), 'hostwords', 'r', 24, 'interleaved', 0, 0, 1, 1, 3, 0),
    ('G48HR', (9, 8), 'hostwords', 'r', 'ulaw', 'channel_major', 0, 0, 1, 0, 1, 0),
    ('G96_25S', (12, 2), 'rates', 'r', 'alaw', 'default', 0, 1, 0, 0, 0, 0),
    ('G48S', (12, 2), 'device', '', 's24_3le', 'default', 0, 0, 0, 0, 0, 0),
    ('G16S', (2, 12), 'host', 'r', 's24_3be', 'channel_major', 0, 0, 0, 1, 0, 0),
    ('G96_25S', (2, 12), 'device', '', 's24_3be', 'interleaved', 1, 0, 1, 0, 1, 0),
    ('G32S', (2, 2), 'host', 'b', 's16be', 'channel_major', 0, 0, 0, 0, 0, 0),
    ('G48S', (12, 12), 'host', 'b', 'ulaw', 'channel_major', 0, 0, 0, 1, 0, 0),
    ('G32S', (48, 9), 'packed', '', 'f32', 'interleaved', 1, 1, 0, 1, 1, 0),
    ('G96_5S', (9, 8), 'device', '', 16, 'default', 0, 0, 1, 1, 3, 0),
    ('G96_25S', (2, 2), 'host', 'r', 32, 'interleaved', 0, 0, 0, 0, 0, 0),
    ('G96_5S', (48, 9), 'hostwords', 'r', 32, 'channel_major', 0, 0, 0, 0, 0, 0),
    ('G96_5S', (2, 2), 'packed', 'r', 24, 'default', 1, 1, 0, 1, 1, 1),
    ('G48S', (9, 8), 'packed', 'rb', 'alaw', 'interleaved', 0, 1, 0, 1, 1, 0),
    ('G48_5S', (2, 2), 'device', '', 16, 'interleaved', 0, 0, 0, 1, 1, 0),
    ('G48', (12, 2), 'host', 'r', 24, 'default', 0, 0, 0, 0, 0, 0),
    ('G32S', (12, 12), 'hostwords', 'r', 'alaw', 'default', 1, 0, 0, 0, 3, 0),
    ('G96S', (12, 12), 'rates', 'r', 'f32', 'interleaved', 1, 0, 1, 1, 0, 0),
    ('G48HR', (2, 12), 'host', 'r', 's24_3be', 'interleaved', 0, 0, 0, 1, 0, 0),
    ('G48_5S', (48, 9), 'device', '', 'ulaw', 'interleaved', 0, 0, 0, 0, 0, 0),
    ('G96S', (2, 12), 'host', 'r', 's24_3le', 'default', 0, 0, 0, 0, 0, 0),
    ('G48HR', (12, 2), 'device', '', 24, 'channel_major', 0, 0, 1, 1, 1, 0),
    ('G48_25S', (48, 9), 'packed', 'r', 'f32', 'interleaved', 0, 0, 1, 0, 3, 1),
    ('G16S', (12, 2), 'packed', 'rb', 'ulaw', 'channel_major', 0, 1, 0, 0, 0, 0),
    ('G44S', (9, 8), 'packed', 'rb', 's16be', 'default', 1, 1, 0, 0, 3, 0),
    ('G44S', (12, 2), 'device', '', 'f32', 'default', 1, 0, 1, 1, 0, 0),
    ('G96_25S', (2, 12), 'packed', 'r', 16, 'interleaved', 1, 0, 1, 1, 3, 1),
    ('G96_5S', (48, 9), 'host', 'r', 'alaw', 'default', 0, 0, 0, 1, 0, 0),
    ('G16S', (12, 12), 'rates', 'b', 's24_3le', 'default', 1, 0, 1, 1, 0, 0),
    ('G48_5S', (9, 8), 'packed', 'b', 24, 'default', 1, 1, 1, 0, 1, 1),
    ('G48HR', (2, 12), 'rates', 'r', 16, 'default', 1, 1, 1, 1, 1, 0),
    ('G32S', (12, 2), 'device', '', 's24_3le', 'default', 1, 0, 1, 0, 1, 0),
    ('G48_25S', (12, 2), 'packed', '', 32, 'interleaved', 0, 1, 1, 1, 1, 1),
    ('G16S', (12, 12), 'packed', 'r', 'alaw', 'interleaved', 1, 1, 0, 0, 0, 1),
    ('G48_5S', (12, 12), 'packed', 'b', 's16be', 'channel_major', 0, 1, 1, 0, 3, 1),
    ('G48S', (9, 8), 'rates', 'b', 's16be', 'default', 1, 1, 1, 0, 3, 0),
    ('G16S', (12, 2), 'hostwords', 'rb', 32, 'default', 0, 0, 1, 1, 0, 0),
    ('G44S', (12, 2), 'rates', 'r', 's24_3be', 'default', 0, 1, 1, 0, 0, 0),
    ('G96S', (48, 9), 'packed', 'r', 'ulaw', 'default', 0, 0, 0, 0, 1, 1),
    ('G48', (2, 2), 'packed', 'rb', 's24_3be', 'interleaved', 0, 1, 1, 1, 1, 0),
    ('G48_25S', (2, 2), 'packed', 'r', 24, 'channel_major', 0, 0, 1, 0, 1, 1),
    ('G96_5S', (2, 2), 'device', '', 's24_3le', 'default', 1, 0, 1, 0, 3, 0),
    ('G44S', (9, 8), 'rates', 'r', 32, 'default', 1, 0, 1, 0, 0, 0),
    ('G96_25S', (12, 2), 'host', 'r', 's24_3le', 'channel_major', 0, 0, 0, 1, 0, 0),
    ('G32S', (12, 12), 'packed', 'r', 'ulaw', 'default', 0, 1, 0, 1, 0, 1),
    ('G48S', (2, 12), 'rates', 'rb', 24, 'channel_major', 0, 1, 1, 1, 0, 0),
    ('G48HR', (2, 12), 'packed', '', 'alaw', 'default', 1, 1, 0, 1, 3, 1),
    ('G48', (2, 2), 'rates', 'b', 's16be', 'default', 0, 1, 0, 1, 1, 0),
    ('G96S', (9, 8), 'device', '', 16, 'default', 1, 0, 1, 1, 3, 0),
    ('G96S', (2, 12), 'hostwords', 'r', 'alaw', 'default', 0, 0, 0, 1, 3, 0),
    ('G96_5S', (2, 2), 'packed', 'r', 'ulaw', 'channel_major', 0, 1, 1, 1, 3, 1),
    ('G48HR', (12, 2), 'packed', '', 'f32', 'interleaved', 1, 1, 1, 1, 1, 0),
    ('G96_25S', (9, 8), 'packed', 'r', 'f32', 'default', 1, 1, 0, 0, 0, 1),
    ('G48_25S', (2, 2), 'packed', 'rb', 's24_3be', 'interleaved', 0, 0, 0, 0, 0, 1),
    ('G48_5S', (12, 12), 'device', '', 32, 'interleaved', 0, 0, 1, 0, 3, 0),
)
DEC_ROWS = (
    ('G48LS', (2, 12), 'hostsizes', 's24_3le', 'channel_major', 0, 0, 0, 0, 0),
    ('G96_5S', (12, 2), 'devhostsizes', 'ulaw', 'default', 1, 0, 1, 1, 1),
    ('G48S', (12, 12), 'packed', 24, 'interleaved', 1, 1, 0, 0, 3),
    ('G96S', (48, 3), 'sizes', 's16be', 'channel_major', 0, 1, 1, 1, 3),
    ('G48', (1, 9), 'device', 'alaw', 'interleaved', 0, 0, 1, 0, 1),
    ('G48_5S', (12, 12), 'host', 's24_3be', 'default', 0, 0, 0, 1, 0),
    ('G16S', (1, 9), 'sizes', 's24_3le', 'default', 1, 1, 0, 0, 1),
    ('G44S', (48, 3), 'devhostsizes', 16, 'interleaved', 1, 0, 0, 0, 0),
    ('G16S', (12, 2), 'packed', 'f32', 'interleaved', 0, 0, 1, 1, 0),
    ('G48HR', (2, 12), 'device', 'alaw', 'default', 1, 0, 0, 1, 3),
    ('G96_25S', (1, 9), 'packed', 32, 'channel_major', 0, 0, 0, 1, 1),
    ('G48HR', (2, 12), 'sizes', 'ulaw', 'interleaved', 0, 1, 1, 0, 0),
    ('G48_25S', (12, 2), 'sizes', 's24_3be', 'channel_major', 0, 1, 1, 0, 3),
    ('G48HR', (12, 12), 'devhostsizes', 24, 'channel_major', 0, 0, 1, 1, 1),
    ('G48_25S', (1, 9), 'devhostsizes', 's16be', 'default', 1, 0, 0, 1, 0),
    ('G96_5S', (12, 12), 'sizes', 32, 'interleaved', 1, 1, 0, 0, 3),
    ('G48LS', (1, 9), 'sizes', 16, 'default', 0, 1, 1, 1, 3),
    ('G96_25S', (48, 3), 'sizes', 'f32', 'default', 1, 1, 1, 0, 3),
    ('G32S', (48, 3), 'packed', 's24_3be', 'default', 1, 1, 1, 1, 1),
    ('G48S', (2, 12), 'device', 16, 'channel_major', 0, 0, 1, 1, 1),
    ('G32S', (2, 12), 'host', 'f32', 'channel_major', 0, 0, 0, 0, 0),
    ('G48LS', (12, 2), 'device', 's16be', 'interleaved', 1, 0, 0, 0, 1),
    ('G44S', (12, 2), 'packed', 's24_3le', 'channel_major', 0, 1, 1, 1, 3),
    ('G48_5S', (2, 12), 'packed', 's16be', 'interleaved', 1, 1, 1, 0, 3),
    ('G96S', (1, 9), 'hostsizes', 24, 'default', 0, 0, 0, 1, 0),
    ('G96_5S', (48, 3), 'packed', 'alaw', 'channel_major', 0, 1, 1, 0, 0),
    ('G48', (12, 12), 'devhostsizes', 's24_3le', 'default', 1, 0, 0, 1, 3),
    ('G96S', (12, 12), 'device', 'ulaw', 'interleaved', 1, 0, 0, 0, 3),
    ('G48_5S', (48, 3), 'device', 32, 'default', 1, 0, 1, 1, 1),
    ('G32S', (12, 12), 'hostsizes', 's16be', 'interleaved', 0, 0, 0, 0, 0),
    ('G48S', (48, 3), 'host', 's24_3le', 'interleaved', 0, 0, 0, 1, 0),
    ('G16S', (12, 2), 'hostsizes', 32, 'channel_major', 0, 0, 0, 1, 0),
    ('G48', (48, 3), 'packed', 'ulaw', 'channel_major', 0, 1, 1, 0, 0),
    ('G96_25S', (2, 12), 'devhostsizes', 's24_3be', 'interleaved', 1, 0, 0, 1, 0),
    ('G44S', (12, 12), 'device', 'f32', 'default', 0, 0, 0, 0, 1),
    ('G96S', (2, 12), 'devhostsizes', 32, 'channel_major', 0, 0, 0, 1, 1),
    ('G48_5S', (12, 2), 'sizes', 24, 'channel_major', 0, 0, 0, 0, 0),
    ('G48S', (1, 9), 'sizes', 'ulaw', 'default', 1, 1, 0, 1, 1),
    ('G32S', (12, 2), 'sizes', 'alaw', 'channel_major', 0, 1, 1, 1, 3),
    ('G48_25S', (2, 12), 'device', 24, 'interleaved', 1, 0, 1, 1, 0),
    ('G48_25S', (12, 12), 'packed', 16, 'default', 1, 0, 1, 0, 1),
    ('G16S', (12, 12), 'devhostsizes', 'alaw', 'channel_major', 0, 0, 1, 0, 3),
    ('G96_25S', (12, 2), 'host', 'ulaw', 'interleaved', 0, 0, 0, 1, 0),
    ('G96_5S', (1, 9), 'host', 's24_3be', 'channel_major', 0, 0, 0, 1, 0),
    ('G48LS', (48, 3), 'host', 32, 'default', 0, 0, 0, 0, 0),
    ('G96_5S', (12, 2), 'hostsizes', 16, 'interleaved', 0, 0, 0, 0, 0),
    ('G48HR', (1, 9), 'hostsizes', 'f32', 'interleaved', 0, 0, 0, 1, 0),
    ('G44S', (2, 12), 'host', 's16be', 'default', 0, 0, 0, 0, 0),
    ('G48LS', (12, 12), 'devhostsizes', 'f32', 'interleaved', 0, 0, 0, 1, 3),
    ('G48_5S', (1, 9), 'devhostsizes', 'alaw', 'interleaved', 0, 0, 1, 0, 1),
    ('G16S', (2, 12), 'device', 's24_3be', 'default', 0, 0, 1, 1, 3),
    ('G16S', (48, 3), 'host', 24, 'channel_major', 0, 0, 0, 0, 0),
    ('G96_5S', (2, 12), 'device', 's24_3le', 'interleaved', 0, 0, 0, 0, 3),
    ('G48', (2, 12), 'sizes', 24, 'interleaved', 1, 1, 0, 1, 1),
    ('G96_25S', (12, 12), 'hostsizes', 16, 'interleaved', 0, 0, 0, 0, 0),
    ('G48_25S', (48, 3), 'hostsizes', 'alaw', 'channel_major', 0, 0, 0, 1, 0),
    ('G96S', (12, 2), 'packed', 'f32', 'default', 1, 1, 0, 0, 0),
    ('G44S', (1, 9), 'hostsizes', 'ulaw', 'default', 0, 0, 0, 0, 0),
    ('G48', (12, 2), 'host', 'f32', 'channel_major', 0, 0, 0, 1, 0),
    ('G48S', (12, 2), 'hostsizes', 's24_3be', 'default', 0, 0, 0, 0, 0),
    ('G48HR', (12, 2), 'host', 's24_3le', 'interleaved', 0, 0, 0, 0, 0),
    ('G48HR', (48, 3), 'packed', 's16be', 'interleaved', 1, 0, 0, 0, 3),
    ('G32S', (1, 9), 'device', 'ulaw', 'interleaved', 0, 0, 1, 1, 1),
    ('G32S', (48, 3), 'devhostsizes', 32, 'interleaved', 1, 0, 1, 1, 1),
    ('G96S', (2, 12), 'host', 'alaw', 'interleaved', 0, 0, 0, 0, 0),
    ('G48_25S', (12, 12), 'host', 's24_3le', 'default', 0, 0, 0, 1, 0),
    ('G96_25S', (48, 3), 'device', 24, 'default', 1, 0, 1, 0, 3),
    ('G16S', (1, 9), 'host', 16, 'default', 0, 0, 0, 0, 0),
    ('G44S', (12, 12), 'sizes', 'alaw', 'default', 1, 1, 1, 0, 0),
    ('G48', (12, 12), 'hostsizes', 32, 'channel_major', 0, 0, 0, 1, 0),
    ('G96S', (12, 2), 'sizes', 16, 'interleaved', 1, 1, 1, 1, 1),
    ('G16S', (1, 9), 'devhostsizes', 'ulaw', 'interleaved', 1, 0, 0, 0, 3),
    ('G48S', (1, 9), 'devhostsizes', 's16be', 'default', 1, 0, 1, 0, 1),
    ('G48_5S', (12, 2), 'hostsizes', 'f32', 'interleaved', 0, 0, 0, 0, 0),
    ('G48LS', (48, 3), 'packed', 'alaw', 'channel_major', 0, 1, 0, 1, 0),
    ('G48LS', (2, 12), 'devhostsizes', 24, 'interleaved', 1, 0, 1, 1, 1),
    ('G32S', (12, 12), 'devhostsizes', 's24_3le', 'interleaved', 1, 0, 0, 1, 0),
    ('G48_5S', (1, 9), 'packed', 16, 'interleaved', 1, 0, 0, 1, 1),
    ('G96_25S', (48, 3), 'packed', 's24_3le', 'interleaved', 0, 0, 0, 1, 0),
    ('G96_5S', (48, 3), 'packed', 's16be', 'channel_major', 0, 1, 0, 0, 3),
    ('G96S', (12, 2), 'device', 's24_3be', 'default', 1, 0, 0, 1, 3),
    ('G48HR', (12, 12), 'device', 's24_3be', 'interleaved', 0, 0, 0, 1, 1),
    ('G48_5S', (1, 9), 'devhostsizes', 'ulaw', 'channel_major', 0, 0, 0, 1, 3),
    ('G48HR', (2, 12), 'packed', 32, 'default', 0, 0, 1, 0, 1),
    ('G48_25S', (12, 2), 'host', 'ulaw', 'interleaved', 0, 0, 0, 1, 0),
    ('G48', (1, 9), 'hostsizes', 's24_3be', 'interleaved', 0, 0, 0, 0, 0),
    ('G48', (2, 12), 'sizes', 's16be', 'default', 1, 0, 0, 1, 0),
    ('G96_25S', (12, 2), 'devhostsizes', 's16be', 'default', 1, 0, 1, 1, 1),
    ('G16S', (12, 2), 'packed', 's16be', 'channel_major', 0, 0, 0, 1, 3),
    ('G96S', (48, 3), 'sizes', 's24_3le', 'interleaved', 0, 1, 0, 1, 3),
    ('G44S', (1, 9), 'host', 32, 'interleaved', 0, 0, 0, 1, 0),
    ('G44S', (12, 12), 'packed', 's24_3be', 'default', 1, 1, 0, 0, 0),
    ('G48_25S', (12, 2), 'devhostsizes', 32, 'interleaved', 0, 0, 0, 0, 3),
    ('G48S', (2, 12), 'packed', 'alaw', 'interleaved', 0, 0, 0, 0, 0),
    ('G96_25S', (48, 3), 'devhostsizes', 'alaw', 'default', 0, 0, 0, 0, 1),
    ('G48S', (12, 12), 'packed', 'f32', 'default', 1, 1, 1, 1, 3),
    ('G96_5S', (12, 12), 'sizes', 'f32', 'channel_major', 0, 0, 0, 0, 3),
    ('G32S', (1, 9), 'host', 16, 'default', 0, 0, 0, 1, 0),
    ('G48', (2, 12), 'packed', 16, 'interleaved', 0, 1, 0, 0, 0),
    ('G48S', (48, 3), 'device', 32, 'default', 1, 0, 0, 1, 0),
    ('G48_5S', (12, 12), 'devhostsizes', 's24_3le', 'default', 1, 0, 0, 0, 3),
    ('G48LS', (12, 12), 'devhostsizes', 'ulaw', 'default', 1, 0, 0, 1, 0),
    ('G32S', (12, 2), 'devhostsizes', 24, 'default', 1, 0, 1, 1, 0),
    ('G48_25S', (12, 2), 'packed', 'f32', 'interleaved', 1, 1, 0, 0, 0),
    ('G48HR', (12, 12), 'sizes', 16, 'default', 1, 1, 1, 1, 1),
    ('G44S', (48, 3), 'devhostsizes', 24, 'default', 0, 0, 1, 0, 3),
    ('G48LS', (2, 12), 'packed', 's24_3be', 'interleaved', 1, 1, 0, 1, 1),
    ('G96_5S', (1, 9), 'devhostsizes', 24, 'channel_major', 0, 0, 0, 1, 3),
)
ROWS = {"enc": ENC_ROWS, "dec": DEC_ROWS}

# launch_resample (lc3_runtime.hip) chooses among seven resamplers by geometry (c->rs48, c->rs96), sample type, layout and pointer alignment AT ONCE, behind
# `placed` and `ragged`, which decide alone: a product of four factors, of which a pair table promises only the pairs (the rows above hold no stereo 48 kHz call
# with wire samples, interleaved, dense and aligned - the one call that shows a missing `!(bitdepth & LC3D_PCM_INTERLEAVED)` in front of
# lc3_enc_resample48w_kernel).  So that function's own factors in full, on the dense device call, 12 frames (pipelined) then 2 (one-wave behind the pre-kernels):
RESAMPLE_GEOMS = ("G48S", "G96_25S")                                        # c->rs48; c->rs96 (N = 240)
RESAMPLE_ROWS = tuple((g, (12, 2), "device", "", form, layout, 0, 0, 0, 0, pad, 0) for g in RESAMPLE_GEOMS for layout in LAYOUTS for form in FORMS for pad in (0, 1, 3))


def _print_tables():
    for side in ("enc", "dec"):
        ex = excluded_by_clause(side)
        print("# %s: valid=%d excluded=%r" % (side, len(valid_pairs(side)), {k: len(v) for k, v in ex.items()}))
        print("%s_ROWS = (" % side.upper())
        for row in generate(side):
            print("    %r," % (row,))
        print(")")


if __name__ == "__main__":
    _print_tables()
