"""tests/option_pairs.py without a GPU: the committed rows are the generator's, every row is valid, the pairs the rows cover are exactly the pairs some valid
call can have (recounted over the whole product of the factors, not with the helper's own search), the tables stay small, every excluded pair belongs to one
named clause, and every clause is what the host does: the format check and the plan functions of the product library, and every batch call of lc3_host.c over
tools/stub_shim.c (`make -C audio_codec_amd/csrc stub`) - which accepts every committed row and refuses every excluded pair of a refusal clause in a call that
breaks that clause alone.  tests/test_gpu_option_pairs.py runs the rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import launch_census as lc
import option_pairs as op
from audio_codec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
SIDES = ("enc", "dec")


@pytest.mark.parametrize("side", SIDES)
def test_committed_rows_are_the_generators(side):
    assert list(op.ROWS[side]) == op.generate(side)


@pytest.mark.parametrize("side", SIDES)
def test_every_row_is_full_and_valid(side):
    fs = op.SIDES[side][0]
    for n, row in enumerate(op.ROWS[side]):
        assert len(row) == len(fs) and all(v in levels for v, (_, levels) in zip(row, fs)), (n, row)
        assert op.violations(side, op.as_dict(side, row)) == [], (n, row)
    assert len(set(op.ROWS[side])) == len(op.ROWS[side])


def test_resample_rows_are_the_whole_product_and_valid():
    rows = op.RESAMPLE_ROWS
    assert len(rows) == len(set(rows)) == len(op.RESAMPLE_GEOMS) * len(op.LAYOUTS) * len(op.FORMS) * 3
    for row in rows:
        r = op.as_dict("enc", row)
        assert op.violations("enc", r) == [] and all(v in levels for v, (_, levels) in zip(row, op.ENC_FACTORS)), row
        assert (r["how"], r["words"], r["placed"], r["ragged"], r["ready"]) == ("device", "", 0, 0, 0) and op.GEOMS[r["geom"]][3] == 2
    assert {(r[0], r[4], r[5], r[10]) for r in rows} == {(g, f, l, p) for g in op.RESAMPLE_GEOMS for f in op.FORMS for l in op.LAYOUTS for p in (0, 1, 3)}


def _product_pairs(side):
    """the valid pairs by brute force: every full row of the product of the factors, the clauses as tables over their two factors, and for each two factors
    the pairs of levels that survive in some row"""
    fs, clauses = op.SIDES[side]
    names = [f for f, _ in fs]
    dims = [len(levels) for _, levels in fs]
    ix = np.indices(dims, dtype=np.int8).reshape(len(dims), -1)
    keep = np.ones(ix.shape[1], bool)
    for c in clauses:
        i, j = names.index(c.fa), names.index(c.fb)
        tab = np.array([[bool(c.hits(a, b)) for b in fs[j][1]] for a in fs[i][1]])
        keep &= ~tab[ix[i], ix[j]]
    ix = ix[:, keep].astype(np.int64)
    pairs = set()
    for i in range(len(dims)):
        for j in range(i + 1, len(dims)):
            seen = np.bincount(ix[i] * dims[j] + ix[j], minlength=dims[i] * dims[j]).reshape(dims[i], dims[j])
            pairs |= {(i, int(a), j, int(b)) for a, b in np.argwhere(seen)}
    return int(np.prod(dims)), int(keep.sum()), pairs


@pytest.mark.parametrize("side", SIDES)
def test_rows_cover_exactly_the_valid_pairs(side):
    n_rows, n_valid_rows, want = _product_pairs(side)
    assert 0 < n_valid_rows < n_rows
    covered = set().union(*(op.row_pairs(side, r) for r in op.ROWS[side]))
    assert covered == want, (sorted(want - covered)[:10], sorted(covered - want)[:10])
    assert want == op.valid_pairs(side)
    print(side, "rows", len(op.ROWS[side]), "of", n_valid_rows, "valid calls; pairs", len(want), "of", len(op.all_pairs(side)))


@pytest.mark.parametrize("side", SIDES)
def test_the_table_stays_small(side):
    """at most 1.3 times the product of the two largest factors, below which no table can go: a group of about ten rows stays a few seconds on the GPU"""
    a, b = sorted(len(levels) for _, levels in op.SIDES[side][0])[-2:]
    assert a * b <= len(op.ROWS[side]) <= int(1.3 * a * b), (len(op.ROWS[side]), a * b)
    assert a * b == {"enc": 99, "dec": 108}[side]


@pytest.mark.parametrize("side", SIDES)
def test_every_excluded_pair_belongs_to_one_clause(side):
    ex = op.excluded_by_clause(side)
    names = [c.name for c in op.SIDES[side][1]]
    assert len(set(names)) == len(names) and all(c.kind in ("refusal", "shape") and c.where for c in op.SIDES[side][1])
    assert set(ex) == set(names), ("a pair without a clause, with two, or a clause that excludes nothing", sorted(map(str, set(ex) ^ set(names))))
    pinned = op.COUNTS[side]
    assert {k: len(v) for k, v in ex.items()} == pinned["excluded"]
    assert len(op.valid_pairs(side)) == pinned["valid"] and len(op.all_pairs(side)) == pinned["pairs"] == pinned["valid"] + sum(pinned["excluded"].values())
    assert set(op.GPU_ONLY_CLAUSES[side]) <= {c.name for c in op.SIDES[side][1] if c.kind == "refusal"}


def test_scenarios_keep_the_thresholds_on_both_sides():
    """the call lengths against the runtime's constants (lc3_plan.h): a call on each side of LC3D_FUSED_MAX_T, and of LC3D_FUSED_MAX_T_READY under the promise"""
    text = open(os.path.join(CSRC, "lc3_plan.h")).read() + open(os.path.join(CSRC, "lc3_runtime.hip")).read()

    def const(name):
        import re
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m, name
        return int(m.group(1))
    t, tr = const("LC3D_FUSED_MAX_T"), const("LC3D_FUSED_MAX_T_READY")
    assert (t + 1, t) in op.ENC_CALLS and op.ENC_CALLS_READY[(t + 1, t)] == (tr + 1, tr)
    assert set(op.ENC_CALLS_READY) == set(op.ENC_CALLS)
    for n, row in enumerate(op.ENC_ROWS):
        sc = op.scenario("enc", n, row)
        r = op.as_dict("enc", row)
        assert sc["calls"] == (op.ENC_CALLS_READY[r["calls"]] if r["ready"] else r["calls"]) and sc["pad"] == r["pad"] * op.ELEM_BYTES[r["form"]]
    # three elements of a type are never a multiple of 16 bytes, and of 4 for the 1- and 3-byte types (launch_resample: resample48 / resample48f, resample48w)
    assert all((3 * b) % 16 and (b not in (1, 3) or (3 * b) % 4) for b in op.ELEM_BYTES.values())
    # stereo geometries have an odd stream-frame size (the census's rule), the new one included
    for name, g in op.GEOMS.items():
        if g[3] == 2:
            assert any(lc.nbytes_of(g[0], 2, g[1], g[2], r) % 2 for r in g[4]), name


# ---- the clauses against the host ----
def _fmt(form, layout):
    return api.pcm_format(api.PCM_FLOAT32 if form == "f32" else form, layout)


def test_format_and_plan_functions_agree_with_the_clauses():
    L = api.load_library()
    for form in op.FORMS:
        for layout in op.LAYOUTS:
            fmt = _fmt(form, layout)                                        # lc3plus_pcm_format_check: every form in every layout is a format
            assert L.lc3plus_pcm_format_check(fmt) == 0 and L.lc3plus_pcm_elem_bytes(fmt) == op.ELEM_BYTES[form]
            # placed_channel_major: lc3plus_plan_placed refuses the layout and nothing else of the two factors
            if layout == "channel_major":
                with pytest.raises(api.LC3Error):
                    api.plan_placed(fmt, 2, 480, np.zeros((3, 2), np.int64), 1 << 20)
                assert api.pcm_placed_offset(fmt, 2, 480, 0, 0, 0) == -1
            else:
                assert not api.plan_placed(fmt, 2, 480, np.zeros((3, 2), np.int64), 1 << 20).any()
    assert L.lc3plus_pcm_format_check(16 | api.PCM_INTERLEAVED | api.PCM_CHANNEL_MAJOR) != 0
    # bandwidth_hr: the rule of encode_device_rates refuses bandwidths for exactly the high-resolution geometries, with or without rates and counts
    for name, (fs, ms, hr, ch, rates) in op.GEOMS.items():
        for words in ("r", "b", "rb"):
            br = np.full((3, 2), rates[0], np.int32) if "r" in words else None
            bw = np.zeros((3, 2), np.int32) if "b" in words else None
            for counts in (None, [2, 0, 1]):
                rc = api.enc_plan_rates_ragged(fs, ch, ms, hr, list(rates), [0, 0, 0], bitrates=br, bandwidths=bw, counts=counts, n_frames=2)[0]
                assert (rc != 0) == ("b" in words and name in op.HR), (name, words, rc)
    # order: lc3plus_plan_packed knows the two orders of the factor
    assert [api.plan_packed(np.ones((3, 2), np.int32), o)[0] for o in (0, 1, 2)] == [0, 0, 1]


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-s", "-C", CSRC, "stub"])
    L = C.CDLL(os.path.join(ROOT, "audio_codec_amd", "_stub", "liblc3plus_stub.so"))
    for name, f in list(vars(api.load_library()).items()):                  # the prototypes api.py declares on the product library
        if name.startswith("lc3") and getattr(f, "argtypes", None) is not None and hasattr(L, name):
            getattr(L, name).argtypes = f.argtypes
            getattr(L, name).restype = f.restype
    return L


P = dict(pcm=0x10000, out=0x20000, br=0x30000, bw=0x40000, nb=0x50000, fl=0x60000, offs=0x70000, cnt=0x80000, tot=0x90000, st=0xA0000, plo=0xB0000)   # stand-ins for device pointers: the host passes them on


def _host_takes(L, side, r):
    """the first call of the row through api.py and lc3_host.c, the HIP side a stub: None if every step is accepted, else the LC3Error"""
    fs, ms, hr, ch, rates = op.GEOMS[r["geom"]]
    S, T = len(rates), r["calls"][0]
    h = C.c_void_p()
    try:
        if side == "enc":
            sizes = [lc.nbytes_of(fs, ch, ms, hr, x) for x in rates]
            assert L.lc3plus_enc_batch_create(C.byref(h), S, fs, ch, ms, hr, (C.c_int * S)(*rates), 0) == 0
            b = api.Batch._borrowed(L, h.value, S, fs, ch, ms, hr)
            fmt = _fmt(r["form"], r["layout"])
            br, bw = lc._words(dict(words=r["words"]), fs, rates, S, T, 0, False)
            if r["ready"]:
                b.set_input_ready(True)
            if r["placed"]:
                b.set_pcm_placement(P["plo"], 1 << 20)
            if r["ragged"]:
                b.set_frame_counts(P["cnt"])
            if r["how"] == "host":
                b.encode(np.zeros(api.pcm_shape(fmt, S, T, ch, b.N), api.pcm_dtype(fmt)), bitdepth=fmt, bitrates=br, bandwidths=bw)
            elif r["how"] in ("device", "hostwords"):
                b.encode_device(P["pcm"], fmt, T, P["out"], max(sizes), bitrates=br, bandwidths=bw)
            elif r["how"] == "rates":
                b.encode_device_rates(P["pcm"], fmt, T, P["out"], max(sizes), P["br"] if br is not None else None, P["bw"] if bw is not None else None, P["nb"], P["fl"])
            else:
                b.encode_device_packed(P["pcm"], fmt, T, P["out"], 1 << 20, r["order"], P["br"] if br is not None else None, P["bw"] if bw is not None else None,
                                       P["offs"], P["tot"], P["nb"], P["fl"])
        else:
            sizes = [lc.nbytes_of(fs, ch, ms, hr, x) for x in rates]
            var = r["how"] in ("hostsizes", "devhostsizes", "sizes", "packed")
            assert L.lc3plus_dec_batch_create(C.byref(h), S, fs, ch, ms, hr, None if var else (C.c_int * S)(*sizes), 0) == 0
            d = api.DecBatch._borrowed(L, h.value, S, ch)
            fmt = _fmt(r["out"], r["layout"])
            nb = np.array(sizes, np.int32)[:, None].repeat(T, axis=1)
            if r["ready"]:
                d.set_input_ready(True)
            if r["placed"]:
                d.set_pcm_placement(P["plo"], 1 << 20)
            if r["ragged"]:
                d.set_frame_counts(P["cnt"])
            if r["how"] in ("host", "hostsizes"):
                d.decode(np.zeros((S, T, max(sizes)), np.uint8), np.zeros((S, T), np.uint8), bps=fmt, num_bytes=nb if var else None)
            elif r["how"] in ("device", "devhostsizes"):
                d.decode_device(P["pcm"], max(sizes), T, P["out"], bps=fmt, num_bytes=nb if var else None)
            elif r["how"] == "sizes":
                d.decode_device_sizes(P["pcm"], max(sizes), T, P["out"], P["nb"], P["fl"], P["st"], bps=fmt)
            else:
                d.decode_device_packed(P["pcm"], 1 << 20, P["offs"], T, P["out"], P["nb"], max(sizes), P["fl"], P["st"], bps=fmt)
        return None
    except api.LC3Error as e:
        return e
    finally:
        if h.value:
            getattr(L, "lc3plus_%s_batch_destroy" % side)(h)


@pytest.mark.parametrize("side", SIDES)
def test_the_host_accepts_every_row(stub, side):
    for n, row in enumerate(op.ROWS[side] + (op.RESAMPLE_ROWS if side == "enc" else ())):
        e = _host_takes(stub, side, op.as_dict(side, row))
        assert e is None, (n, row, str(e))


@pytest.mark.parametrize("side", SIDES)
def test_the_host_refuses_every_excluded_pair_of_a_refusal_clause(stub, side):
    """each in a call that breaks that clause alone, so the refusal is the clause's; the same call with either level of the pair moved to one the clause
    allows is accepted"""
    ex = op.excluded_by_clause(side)
    done = 0
    for c in op.SIDES[side][1]:
        if c.kind != "refusal" or c.name in op.GPU_ONLY_CLAUSES[side]:
            continue
        for p in ex[c.name]:
            r = op.only_breaks(side, p, c.name)
            assert r is not None and op.violations(side, r) == [c.name], (c.name, p)
            e = _host_takes(stub, side, r)
            assert isinstance(e, api.LC3Error), (c.name, r)
            mended = 0
            for f in (c.fa, c.fb):
                for v in dict(op.SIDES[side][0])[f]:
                    r2 = dict(r, **{f: v})
                    if op.valid(side, r2):
                        assert _host_takes(stub, side, r2) is None, (c.name, r2)
                        mended += 1
                        break
            assert mended, (c.name, r)
            done += 1
    assert done == sum(len(ex[c.name]) for c in op.SIDES[side][1] if c.kind == "refusal")
