"""CPU: the call-shape restatement of call_shapes.py - that its constants are the sources' (#defines and defaults of lc3_runtime.hip, lc3_launch.h, lc3_plan.h),
that over all sequences every shape rule has a call below it, at it and above it and every grid tail its remainders 0, 1 and unit - 1 in every kernel family the
rule applies to, that the inputs hold what the sequences are there for (by the oracle and api.frame_info_side alone), and that enc_pipelined makes exactly R runs
for every call length with the default run lengths."""
import os
import re

import numpy as np
import pytest

import call_shapes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^\s*#define\s+%s\s+(\d+)\b" % re.escape(name), text, re.M)
    assert m, name
    return int(m.group(1))


# ---- constants ----------------------------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    rt, la, pl = _src("lc3_runtime.hip"), _src("lc3_launch.h"), _src("lc3_plan.h")
    for name in ("LC3D_RUN_FRAMES", "LC3D_RUN_FRAMES_READY", "LC3D_MAX_RUNS", "LC3D_FUSED_MAX_T", "LC3D_FUSED_MAX_T_READY", "LC3D_AHEAD_MAX_FRAMES", "LC3D_SETS",
                 "DEC_SETS"):
        assert _define(rt, name) == getattr(cs, name), name
    for name in ("WAVE", "FRONT_FPW", "FM_F240", "IMDCT_FPW", "RATE_WG"):
        assert _define(la, name) == getattr(cs, name), name
    assert _define(pl, "LC3D_PLAN_HEAD_WORDS") == 45 and "int pc[LC3D_PLAN_HEAD_WORDS];" in la
    # sizeof(ParseLds): every member of the struct as the source declares it (a member added or resized changes the sum)
    body = re.search(r"struct __attribute__\(\(aligned\(16\)\)\) ParseLds \{(.*?)\n\};", la, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for m in body.split(";") if m.strip()]
    width = {"unsigned short": 2, "unsigned char": 1, "unsigned": 4, "int": 4}
    total = 0
    for m in members:
        ty, name, dim = re.fullmatch(r"(unsigned short|unsigned char|unsigned|int) (\w+)\[([^\]]+)\]", m).groups()
        total += width[ty] * eval(dim, {"LC3D_PLAN_HEAD_WORDS": _define(pl, "LC3D_PLAN_HEAD_WORDS")})
    assert len(members) == 5 and total == cs.PARSE_STATIC_BYTES, (members, total)
    assert "q->wpg = (int)((64 * 1024 - sizeof(ParseLds)) / q->per_wave);" in rt and "const int nlw = (WS_ROW(c->N) / 2 + 31) / 32;" in rt
    assert "q->per_wave = (size_t)(q->nw_max + nlw) * WAVE * sizeof(unsigned);" in rt and "#define WS_ROW(N) ((N) > 480 ? 960 : 480)" in pl
    # the defaults of read_opts and the rules written into the launch code
    assert 'o->pre_runs = env_int("LC3PLUS_ENC_PRE_RUNS", 1, 64, %d);' % cs.PRE_RUNS in rt
    assert 'o->pack_wpg = env_int("LC3PLUS_ENC_PACK_WPG", 1, 4, %d);' % cs.PACK_WPG in rt
    assert "c->N == 480 && dT >= %d && c->max_nbytes <= %d)" % (cs.W5_MIN_FRAMES, cs.W5_MAX_BYTES) in rt
    assert "!c->big && (c->mean_nbytes >= %d || n_frames <= %d))" % (cs.RATE_MEAN_BYTES, cs.RATE_SHORT_CALL) in rt
    assert "!(c->big || (c->mean_nbytes < %d && n_frames >= %d && n_frames <= %d && (n_frames & %d) == 0))" % (
        cs.RATE_MEAN_BYTES, cs.RATE_FRONT_LO, cs.RATE_FRONT_HI, cs.RATE_FRONT_MASK) in rt
    assert "(c->hr && c->N == %d && n_frames >= %d)" % (cs.SHAPE_ON_PITCH_N, cs.SHAPE_ON_PITCH_FRAMES) in rt
    assert "q->max_nb > %d ? 0" % cs.PARSE_LDS_MAX_BYTES in rt and "if (q->wpg > %d) q->wpg = %d;" % (cs.PARSE_MAX_WPG, cs.PARSE_MAX_WPG) in rt
    assert "const dim3 grid((unsigned)((n + %d) / %d)), block(%d);" % (cs.PLAN_WG - 1, cs.PLAN_WG, cs.PLAN_WG) in rt                      # dec_plan
    assert "dim3((unsigned)((n + %d) / %d)), dim3(%d), 0, s, c->d_sizes" % (cs.PLAN_WG - 1, cs.PLAN_WG, cs.PLAN_WG) in rt      # dec_tail
    assert "(nt + 3) / 4)), dim3(WAVE), 0, c->s_fr" in rt and cs.FRONT4_FPW == 4                                              # front4: four frames a wave
    assert "((n_frames + 3) / 4)))" in rt and cs.IMDCT4_FPW == 4                                                              # imdct4
    assert "(plan->N > 120 ? FM_F240 : %d) : 0;" % cs.FM_SHORT in rt
    assert "hn0 = r->hk == 0 ? Tr : prn * Tr" in rt                                                                           # the first run, then pre_runs runs at a time
    assert "s->nbLost < 4 ? 1.0 : s->nbLost < %d ? 0.9 : 0.85" % cs.PLC_RAMP in open(os.path.join(ROOT, "oracle", "lc3_oracle_dec.inc")).read()


def test_the_sequences_are_what_the_rules_give():
    assert cs.enc_ordered_lengths() == [1, 8, 9, 15, 16, 17, 32, 33, 47, 48, 49, 64, 65, 128, 129, 256, 257, 273] and sum(cs.enc_ordered_lengths()) == 1447
    assert cs.enc_count_lengths() == [1, 9, 17, 48]
    assert cs.enc_ready_blocks() == [5, 6, 7, 17, 63, 64, 65, 129, 256, 257] and cs.ENC_READY_REPEAT == 5
    assert cs.dec_ordered_lengths() == [1, 3, 4, 5, 7, 8, 9, 16, 17, 33, 64, 65, 129]
    assert cs.dec_whole_wg_lengths() == [255, 256, 257] and cs.dec_count_lengths() == [1, 5, 9] and cs.dec_ready_blocks() == [1, 3, 4, 5, 9, 17]
    for name in ("enc_ordered", "enc_count", "dec_ordered", "dec_whole", "dec_count"):
        assert len(set(cs.sequence(name))) == len(cs.sequence(name))
    assert sorted(set(cs.sequence("enc_ready"))) == cs.enc_ready_blocks() and len(cs.sequence("enc_ready")) == 50
    assert sorted(set(cs.sequence("dec_ready"))) == cs.dec_ready_blocks() and len(cs.sequence("dec_ready")) == 36
    g = cs.enc_geometry
    assert list(ENC.keys()) == ["48k_10_small", "48k_10_large", "48k_5_stereo", "48k_2p5", "32k_10", "96k_2p5_hr", "96k_10", "16k_2p5"]
    assert cs.enc_tail_lengths() == [20, 24, 25, 255, 256, 257] and [g(n)["nbytes"] for n in cs.ENC_TAIL_BATCHES] == [[cs.W5_MAX_BYTES], [cs.W5_MAX_BYTES + 1]]
    assert cs.front_of(g("16k_2p5")) == ("lc3_enc_frontm_kernel", cs.FM_SHORT) and cs.front_of(g("48k_5_stereo")) == ("lc3_enc_frontm_kernel", cs.FM_F240)
    assert all(cs.enc_geometry(n)["S"] == 5 for n in list(ENC) + list(cs.ENC_READY_FAMILIES))
    assert [cs.enc_geometry(n)["ncs"] for n in cs.ENC_COUNT_BATCHES] == [1, 2, 63, 64, 65, 6]
    assert (max(g("48k_10_small")["chan_bytes"]) <= cs.W5_MAX_BYTES and g("48k_10_small")["mean_nbytes"] < cs.RATE_MEAN_BYTES and not g("48k_10_small")["any_attack"])
    assert g("48k_10_large")["mean_nbytes"] >= cs.RATE_MEAN_BYTES and g("48k_10_large")["any_attack"] and g("32k_10")["any_attack"]
    assert [n for n in ENC if g(n)["any_attack"]] == ["48k_10_large", "32k_10"]
    assert all(n % 2 for n in g("48k_5_stereo")["nbytes"]) and g("96k_10")["big"] and not g("96k_2p5_hr")["big"] and g("96k_2p5_hr")["N"] == 240


ENC = cs.ENC_FAMILIES


def test_run_lengths_of_the_named_calls():
    runs = lambda n, **kw: cs.enc_runs(n, **kw)[2]
    assert runs(17) == [9, 8] and runs(33) == [11, 11, 11] and runs(49) == [13, 13, 13, 10] and runs(257) == [17] * 15 + [2] and runs(273) == [18] * 15 + [3]
    assert runs(65, ready=True) == [33, 32] and runs(256, ready=True) == [64] * 4 and cs.enc_runs(257, ready=True)[0] == 5
    g = cs.enc_geometry("48k_10_small")
    pieces = {n: cs.enc_shape(g, n)["pieces"] for n in cs.enc_ordered_lengths()}
    assert min(n for n, p in pieces.items() if p == 3) == 65 and pieces[64] == 2 and pieces[16] == 1 and pieces[257] == 6
    # LC3PLUS_ENC_RUN_FRAMES = 1 and 3 at 9, 18, 35 frames: runs of 1, 2 and 3 frames
    assert runs(9, run_frames=1) == [1] * 9 and runs(18, run_frames=1) == [2] * 9 and runs(35, run_frames=1) == [3] * 11 + [2]
    assert runs(9, run_frames=3) == [3] * 3 and runs(18, run_frames=3) == [3] * 6 and runs(35, run_frames=3) == [3] * 11 + [2]


def test_the_orders_hand_every_path_to_every_other():
    g = cs.enc_geometry("48k_10_small")
    sh = cs.enc_shapes(g, cs.sequence("enc_ordered"))
    pairs = {(a["path"], a["writer"], b["path"], b["writer"]) for a, b in zip(sh, sh[1:])}
    W, W5 = cs.WRITERS
    for want in (("pipelined", W5, "one_wave", None), ("pipelined", W, "one_wave", None), ("one_wave", None, "pipelined", W), ("one_wave", None, "pipelined", W5),
                 ("pipelined", W5, "pipelined", W), ("pipelined", W, "pipelined", W5)):
        assert want in pairs, want
    steps = [(a["n"], b["n"]) for a, b in zip(sh, sh[1:])]
    assert any(a < b for a, b in steps) and any(a > b for a, b in steps)
    assert any(len(a["runs"]) > len(b["runs"]) > 1 for a, b in zip(sh, sh[1:])) and any(1 < len(a["runs"]) < len(b["runs"]) for a, b in zip(sh, sh[1:]))
    for seq in ("dec_ordered", "dec_ready", "dec_count"):
        L = cs.sequence(seq)
        k = cs.role3_calls(L)
        assert 1 in L[k:k + 3] and max(L[k:k + 3]) > cs.PLC_RAMP


# ---- the census of rules --------------------------------------------------------------------------------------------------------------------------------------
NOT_48K_10 = "enc_writer: w5 needs !c->big && !c->hr && c->N == 480"
LARGE_FRAMES = "enc_writer: w5 needs c->max_nbytes <= 100; the family's frames have 160 ... 400 bytes"
MEAN_120 = "enc_pipelined: with c->mean_nbytes >= 120 want_rt holds whatever n_frames is, and on_pre's exception needs mean_nbytes < 120"
BIG = "enc_pipelined: want_rt needs !c->big, on_pre is false for c->big"
NOT_HR_240 = "enc_run: sop needs c->hr && c->N == 240"
# (rule, family) the family cannot reach, each with the line that shows why; test_census_of_rules asserts that they are unmet
UNREACHABLE = {}
for _f in ENC:
    _g = cs.enc_geometry(_f)
    if _g["big"] or _g["hr"] or _g["N"] != 480:
        UNREACHABLE[("w5", _f)] = NOT_48K_10
    elif _g["max_nbytes"] > cs.W5_MAX_BYTES:
        UNREACHABLE[("w5", _f)] = LARGE_FRAMES
    if _g["big"]:
        UNREACHABLE[("rate_short", _f)] = UNREACHABLE[("rate_front", _f)] = BIG
    elif _g["mean_nbytes"] >= cs.RATE_MEAN_BYTES:
        UNREACHABLE[("rate_short", _f)] = UNREACHABLE[("rate_front", _f)] = MEAN_120
    if not (_g["hr"] and _g["N"] == cs.SHAPE_ON_PITCH_N):
        UNREACHABLE[("shape_stream", _f)] = NOT_HR_240
def _ordered(fam):
    return cs.enc_shapes(cs.enc_geometry(fam), cs.sequence("enc_ordered"))


def _threshold(values, below, at, above):
    return {"below": any(below(v) for v in values), "at": any(at(v) for v in values), "above": any(above(v) for v in values)}


def _rule_reach(fam):
    """{rule: {below, at, above}} of the ordered sequence on one family, by the restatement's decisions (not by the lengths alone)"""
    g, sh = cs.enc_geometry(fam), _ordered(fam)
    by_n = {s["n"]: s for s in sh}
    ns = sorted(by_n)
    out = {}
    T = cs.LC3D_FUSED_MAX_T
    out["one_wave"] = {"below": any(n < T and by_n[n]["path"] == "one_wave" for n in ns), "at": by_n[T]["path"] == "one_wave", "above": by_n[T + 1]["path"] == "pipelined"}
    r = cs.LC3D_RUN_FRAMES
    out["runs"] = {"below": len(by_n[r - 1]["runs"]) == 1, "at": len(by_n[r]["runs"]) == 1 and len(by_n[2 * r]["runs"]) == 2,
                   "above": by_n[r + 1]["runs"] == [9, 8] and len(by_n[2 * r + 1]["runs"]) == 3}
    cap = cs.LC3D_MAX_RUNS * r
    out["max_runs"] = {"below": any(len(by_n[n]["runs"]) < cs.LC3D_MAX_RUNS for n in ns if n > r), "at": by_n[cap]["runs"] == [r] * cs.LC3D_MAX_RUNS,
                       "above": by_n[cap + 1]["Tr"] == r + 1 and len(by_n[cap + 1]["runs"]) == cs.LC3D_MAX_RUNS and any(by_n[n]["Tr"] == r + 2 for n in ns)}
    out["pieces"] = {"below": by_n[r]["pieces"] == 1, "at": by_n[4 * r]["pieces"] == 2, "above": by_n[4 * r + 1]["pieces"] == 3}
    out["last_run_shorter"] = {"below": any(s["runs"] and s["runs"][-1] == s["Tr"] for s in sh), "at": any(s["runs"] and s["runs"][-1] == s["Tr"] - 1 for s in sh),
                               "above": any(s["runs"] and s["runs"][-1] < s["Tr"] - 1 for s in sh)}
    pipe = [s for s in sh if s["path"] == "pipelined"]
    S = cs.RATE_SHORT_CALL
    out["rate_short"] = {"below": any(s["n"] < S and s["rate_stream"] != "caller" for s in pipe), "at": by_n[S]["rate_stream"] != "caller",
                         "above": by_n[S + 1]["rate_stream"] == "caller"}
    lo = cs.RATE_FRONT_LO
    out["rate_front"] = {"below": by_n[lo - 1]["rate_stream"] == "pitch", "at": by_n[lo]["rate_stream"] == "front", "above": by_n[lo + 1]["rate_stream"] == "pitch"}
    P = cs.SHAPE_ON_PITCH_FRAMES
    out["shape_stream"] = {"below": any(s["n"] < P and s["shape_stream"] == "front" for s in pipe), "at": by_n[P]["shape_stream"] == "pitch",
                           "above": by_n[P + 1]["shape_stream"] == "pitch"}
    W = cs.W5_MIN_FRAMES
    out["w5"] = {"below": by_n[W - 1]["writer"] == cs.WRITERS[0], "at": by_n[W]["writer"] == cs.WRITERS[1], "above": by_n[W + 1]["writer"] == cs.WRITERS[1]}
    return out


@pytest.mark.parametrize("fam", list(ENC))
def test_census_of_rules(fam):
    for rule, reach in _rule_reach(fam).items():
        if (rule, fam) in UNREACHABLE:
            assert not (reach["at"] and reach["above"] and reach["below"]), (rule, fam, "listed as unreachable, but reached")
            continue
        assert all(reach.values()), (rule, fam, reach)


def test_census_of_rules_under_the_promise():
    for fam in cs.ENC_READY_FAMILIES:
        g = cs.enc_geometry(fam)
        sh = cs.enc_shapes(g, cs.sequence("enc_ready"), ready=True)
        by_n = {}
        for s in sh:
            by_n.setdefault(s["n"], []).append(s)
        q = cs.LC3D_FUSED_MAX_T_READY
        assert by_n[q][0]["path"] == "one_wave" and by_n[q + 1][0]["path"] == "pipelined"        # (the blocks hold no call below 5 frames)
        R = cs.LC3D_RUN_FRAMES_READY
        assert by_n[R - 1][0]["runs"] == [R - 1] and by_n[R][0]["runs"] == [R] and by_n[R + 1][0]["runs"] == [33, 32] and len(by_n[2 * R + 1][0]["runs"]) == 3
        a = cs.LC3D_AHEAD_MAX_FRAMES
        # the first call of a block is ordered (the length changed), the four behind it overlap - up to 256 frames, not from 257; a one-wave call never overlaps
        for n, calls in by_n.items():
            assert [c["overlaps"] for c in calls] == [False] + [n <= a and n > q] * (cs.ENC_READY_REPEAT - 1), (fam, n)
        assert len(by_n[a][0]["runs"]) == 4 and len(by_n[a + 1][0]["runs"]) == 5
        # every set of hand-over buffers is used again inside a block
        assert cs.ENC_READY_REPEAT > cs.LC3D_SETS and cs.DEC_READY_REPEAT >= 2 * cs.DEC_SETS


def _rem(values, unit):
    return {v % unit for v in values}


def test_census_of_grid_tails():
    want = lambda unit: {0, 1, unit - 1}
    calls = cs.all_enc_calls()
    pipe = [(n, s) for n, s in calls if s["path"] == "pipelined"]
    # the fronts, per kernel: frames of a run against the frames a wave takes - inside each run, so a call of whole groups still cuts them (49: 13 + 13 + 13 + 10)
    # (lc3_enc_frontm_kernel takes fm_frames = 4 frames a wave at N = 240 and 8 at N = 40: both)
    for front, unit in ((cs.FRONTS[0], cs.FRONT4_FPW), (cs.FRONTS[1], cs.FM_F240), (cs.FRONTS[1], cs.FM_SHORT), (cs.FRONTS[2], cs.FRONT_FPW), (cs.FRONTS[3], cs.FRONT_FPW)):
        mine = [s for _, s in pipe if s["front"] == front and s["fpw"] == unit]
        nts = [nt for s in mine for nt in s["runs"]]
        assert _rem(nts, unit) >= want(unit), (front, unit, sorted(_rem(nts, unit)))
        assert any(len(s["runs"]) > 1 and any(nt % unit for nt in s["runs"][:-1]) for s in mine), (front, unit)      # a group cut inside a call
    assert cs.FM_F240 != cs.FM_SHORT
    small = [s for n, s in pipe if n == "48k_10_small" and s["Tr"] <= 3]
    assert {nt for s in small for nt in s["runs"]} == {1, 2, 3}                                 # nt < FRONT_FPW, front groups cut inside every run
    # the lane kernels (one source for every family): 64 (stream, frame) pairs per wave over ncs * nt
    lanes = [cs.enc_geometry(n)["ncs"] * nt for n, s in pipe for nt in s["runs"]]
    assert _rem(lanes, cs.WAVE) >= want(cs.WAVE), sorted(_rem(lanes, cs.WAVE))                    # (63: 63 streams in runs of one frame)
    ncs = [cs.enc_geometry(n)["ncs"] for n, s in pipe]
    assert _rem(ncs, 2) == {0, 1}                                                                 # pitch2: pairs of channel-streams
    assert _rem(ncs, cs.RATE_WG) >= want(cs.RATE_WG)                                              # the rate kernel: RATE_WG streams per workgroup
    assert _rem(ncs, cs.WAVE) >= want(cs.WAVE)                                                    # HP50: 64 streams per wave
    assert _rem([cs.enc_geometry(n)["ncs"] for n, s in pipe if cs.enc_geometry(n)["any_attack"]], cs.WAVE) >= want(cs.WAVE)      # the attack kernel
    wg = cs.PACK_WPG * cs.WAVE
    for writer in cs.WRITERS:                                                                     # each writer: wpg * 64 frames per workgroup over ncs * dT
        tasks = _rem([cs.enc_geometry(n)["ncs"] * s["n"] for n, s in pipe if s["writer"] == writer], wg)
        assert tasks >= want(wg), (writer, sorted(tasks))
    # ... and the five-wave writer's size limit at it and above it: one stream of 100 bytes takes it, one of 101 does not
    by = {n: {s["writer"] for m, s in pipe if m == n and s["n"] >= cs.W5_MIN_FRAMES} for n in cs.ENC_TAIL_BATCHES}
    assert by == {"one_100B": {cs.WRITERS[1]}, "one_101B": {cs.WRITERS[0]}}
    # the second rate-stream rule's upper end (the ordered lengths hold its lower end: _rule_reach): inside, at its end, above it
    for name in cs.ENC_TAIL_BATCHES:
        rs = {s["n"]: s["rate_stream"] for m, s in pipe if m == name}
        assert (rs[cs.RATE_FRONT_HI - 4], rs[cs.RATE_FRONT_HI], rs[cs.RATE_FRONT_HI + 1]) == ("front", "front", "pitch"), (name, rs)
    # the decoder
    L = cs.sequence("dec_ordered")
    assert _rem(L, cs.IMDCT4_FPW) >= want(cs.IMDCT4_FPW) and _rem(L, cs.IMDCT_FPW) >= want(cs.IMDCT_FPW)
    assert _rem([n for n in cs.sequence("dec_whole")], cs.PLAN_WG) == want(cs.PLAN_WG)            # one stream: a whole parse, plan and tail workgroup
    g = cs.dec_geometry("48k_10_80B")
    assert cs.dec_shape(g, 256, "sizes", 80)["wpg"] * cs.WAVE == cs.PLAN_WG
    assert _rem(DEC_COUNTS, cs.WAVE) == want(cs.WAVE)                                             # lc3_dec_plc_kernel: 64 streams per wave
    assert _rem(cs.sequence("dec_count"), cs.IMDCT4_FPW) >= {1} and len(cs.sequence("dec_count")) == 3


DEC_COUNTS = (63, 64, 65)


def test_the_decoder_restatement_names_the_kernels():
    for fam, parser, imdct in (("48k_10_80B", "lc3_dec_parse_kernel", "lc3_dec_imdct4_kernel"), ("48k_10_160B", "lc3_dec_parse_kernel_g", "lc3_dec_imdct4_kernel"),
                               ("48k_10_stereo", "lc3_dec_parse_kernel", "lc3_dec_imdct4_kernel"), ("32k_5", "lc3_dec_parse_kernel", "lc3_dec_imdct_kernel"),
                               ("96k_10", "lc3_dec_parse_kernel_g", "lc3_dec_imdct_kernel_big")):
        g = cs.dec_geometry(fam)
        sh = cs.dec_shape(g, 9, "fixed", max(g["chan_bytes"]))
        assert (sh["parser"], sh["imdct"], sh["wpg"]) == (parser, imdct, 4), fam
        assert cs.dec_shape(g, 9, "sizes", max(g["chan_bytes"]))["parser"] == parser + "_var"
        e = cs.expected_launches("dec", g, sh)
        assert sum(e.values()) == 2 and set(e) == set(cs.DEC_KERNELS)
    e = cs.expected_launches("enc", cs.enc_geometry("96k_10"), cs.enc_shape(cs.enc_geometry("96k_10"), 65))
    assert e == dict(dict.fromkeys(cs.ENC_KERNELS, 0), **{"lc3_enc_rate_kernel_big": 5, "lc3_enc_front_kernel_big": 5, "lc3_enc_pack_kernel": 1, "lc3_enc_hp50_kernel": 3})


def test_no_frame_takes_fewer_parse_waves():
    """every channel frame size of both row widths gives PARSE_MAX_WPG waves per parse workgroup: the wpg formula has no smaller result to exercise"""
    for N in (480, 960):
        got = {cs.parse_wpg(N, nb)[1] for nb in range(0, 626)}
        assert got == {cs.PARSE_MAX_WPG}, (N, got)
    assert (32 + 15) * cs.WAVE * 4 * cs.PARSE_MAX_WPG + cs.PARSE_STATIC_BYTES + 15 <= 64 * 1024


# ---- the census of inputs -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(cs.DEC_FAMILIES))
def test_loss_roles_give_the_status_they_say(fam):
    c = cs.dec_case(fam, "dec_ordered")
    _, st = cs.oracle_decode(fam, "dec_ordered")
    L, lost = c["lengths"], c["lost"]
    b = cs.starts(L)
    assert (st == cs.expected_status(L, c["g"]["S"])).all(), np.argwhere(st != lost)[:6].tolist()
    assert not lost[0].any()                                                                      # 1: no loss
    for k in range(len(L)):
        a, e = int(b[k]), int(b[k + 1])
        assert lost[1, e - 1] == (k + 1 < len(L)) or L[k] == 1
        assert lost[1, a] == (k > 0) or L[k] == 1                                                 # 2: the last frame of every call and the first of the next
        assert lost[1, a + 1:e - 1].sum() == 0
        assert lost[3, a] and not lost[3, a + 1:e].any()                                          # 4: only the first frame of every call
        assert lost[4, max(a, e - 2):e].all() and not lost[4, a:max(a, e - 2)].any()              # 5: the last two frames of every call
    k3 = cs.role3_calls(L)
    a, e = int(b[k3]), int(b[k3 + 3])
    assert lost[2, a:e].all() and lost[2].sum() == e - a and 1 in L[k3:k3 + 3]                    # 3: every frame of three consecutive calls
    # ... and the per-frame factor has taken its last value (the eighth lost frame) before the burst ends, inside a call and not at its last frame
    assert e - a > cs.PLC_RAMP + 1 and max(L[k3:k3 + 3]) > cs.PLC_RAMP
    # role 4 leaves DST_QPREV to a previous call whose last good frame was its last frame, for calls of length 0, 1 and 3 modulo 4
    assert {n % 4 for n in L} >= {0, 1, 3}
    # role 5: the frame DST_QPREV is taken from is not the launch's last, and the first frame of the next call is good
    assert all(not lost[4, int(b[k])] for k in range(1, len(L)) if L[k] > 2)
    if c["g"]["ch"] == 2:
        s = cs.STEREO_CORRUPT_STREAM
        assert (c["payload_lost"][s] == lost[s]).all() and not c["bfi"][s].any() and c["payload_lost"].sum() == lost[s].sum()
    else:
        assert not c["payload_lost"].any() and (c["bfi"] == lost).all()


@pytest.mark.parametrize("fam", cs.DEC_READY_FAMILIES)
def test_refused_payloads_stand_for_the_flags_under_the_promise(fam):
    c = cs.dec_case(fam, "dec_ready", None, 0, True)
    _, st = cs.oracle_decode(fam, "dec_ready", None, 0, True)
    assert not c["bfi"].any() and (c["payload_lost"] == c["lost"]).all() and (st == c["lost"]).all()
    assert c["lost"][1:].any(axis=1).all() and not c["lost"][0].any()


@pytest.mark.parametrize("fam", [f for f in cs.DEC_FAMILIES if cs.dec_geometry(f)["ltpf"][1 * cs.dec_geometry(f)["ch"]]])
def test_the_pitched_stream_keeps_the_ltpf_running_across_boundaries(fam):
    """stream 1 (boundary losses): at some boundary the last good frame in front of the burst and the first good frame behind it both have the filter active - the
    two frames at the boundary itself are lost, their payloads never parsed, so the filter crosses the boundary through the concealment, which keeps it running"""
    c = cs.dec_case(fam, "dec_ordered")
    L = c["lengths"]
    b = cs.starts(L)
    act = np.array([cs.ltpf_active(c, 1, t) for t in range(int(b[-1]))])
    around = [k for k in range(1, len(L)) if L[k - 1] >= 3 and L[k] >= 3 and act[b[k] - 2] and act[b[k] + 1] and not c["lost"][1, b[k] - 2] and not c["lost"][1, b[k] + 1]]
    assert around and all(c["lost"][1, b[k] - 1] and c["lost"][1, b[k]] for k in around), (fam, around, int(act.sum()))


def test_families_without_ltpf_are_the_ones_the_rule_switches_it_off_in():
    assert [f for f in cs.DEC_FAMILIES if not cs.dec_geometry(f)["ltpf"][cs.dec_geometry(f)["ch"]]] == ["48k_10_160B", "96k_10"]


@pytest.mark.parametrize("fam", [f for f in ENC if cs.enc_geometry(f)["any_attack"]])
def test_onsets_fall_on_the_first_and_the_last_frame_of_a_call(fam):
    L = cs.sequence("enc_ordered")
    b = cs.starts(L).tolist()
    first, last = cs.onset_frames(L)
    assert first in b[1:-1] and last + 1 in b[1:] and b.index(first) != b.index(last + 1) - 1
    att = cs.attack_flags(fam, "enc_ordered")
    g = cs.enc_geometry(fam)
    handled = [i for i, n in enumerate(g["chan_bytes"]) if cs._api().plan_chan(g["fs"], g["ms"], g["hr"], n)["attack_handling"]]
    assert handled and att[handled, first].all() and att[handled, last].all() and not att[handled, first - 1].any() and not att[handled, last - 1].any()


# ---- the run invariant ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ready", [False, True])
def test_enc_pipelined_makes_exactly_R_runs(ready):
    """enc_pipelined loops tb = 0, Tr, 2 Tr ... below n: ceil(n / Tr) runs.  With the default run lengths that is R for every n, so the index of the last run a call
    made (what an overlapped successor waits on) is R - 1; with LC3PLUS_ENC_RUN_FRAMES = 1 it is not (n = 20: R = 16, Tr = 2, ten runs)."""
    n = np.arange(1, 100001, dtype=np.int64)
    runf = cs.LC3D_RUN_FRAMES_READY if ready else cs.LC3D_RUN_FRAMES
    R = np.clip(-(-n // runf), 1, cs.LC3D_MAX_RUNS)
    Tr = -(-n // R)
    made = -(-n // Tr)
    assert (made == R).all(), n[made != R][:8].tolist()
    for k in (1, 15, 16, 17, 255, 256, 257, 273, 4096, 99999):
        assert cs.enc_runs(k, ready)[0] == len(cs.enc_runs(k, ready)[2]) == int(R[k - 1])
    assert cs.enc_runs(20, run_frames=1)[:2] == (16, 2) and len(cs.enc_runs(20, run_frames=1)[2]) == 10
