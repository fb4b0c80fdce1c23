"""Every pair of options of one call on the GPU (tests/option_pairs.py: ENC_ROWS, DEC_ROWS).  One case per geometry and side, about ten rows each: every row
runs through the census engines (tests/launch_census.py: run_encoder, run_decoder) inside api.launch_census() - what it wrote equals the CPU oracle frame by
frame, num_bytes, flags and status are the host plan's, and every byte a call may not write holds its sentinel.  A failing row is named by its number in the
table.  Then the refusals: one excluded pair of every refusal clause as a call that breaks that clause alone, on real buffers - it raises LC3Error, every
output keeps its sentinels, and the scenario that follows on the same batch (the same row with the clause mended) equals the oracle.  (Every one of them is
refused by lc3_host.c before the runtime is asked, option_pairs.GPU_ONLY_CLAUSES is empty; here they run against the real runtime all the same.)

LC3PLUS_OPTION_PAIRS_RECORD=<file>: the entry points every row launched are appended there, one line per row (profiles/option_pairs_launches.txt is such a
record: which rows reach which twin).  A record, not an assertion."""
import os

import numpy as np
import pytest

import launch_census as lc
import option_pairs as op
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu

GROUPS = [(side, geom) for side in ("enc", "dec") for geom in op.SIDES[side][0][0][1]]


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _run(dev, amd, sc):
    with amd.api.launch_census() as census:
        (lc.run_encoder if sc["kind"] == "enc" else lc.run_decoder)(dev, sc, amd)
    return census


@pytest.mark.parametrize("side,geom", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_rows_equal_the_oracle(dev, side, geom):
    amd = _amd()
    rows = [(n, row) for n, row in enumerate(op.ROWS[side]) if row[0] == geom]
    assert 6 <= len(rows) <= 14, len(rows)
    failed, record = [], []
    for n, row in rows:
        sc = op.scenario(side, n, row)
        try:
            census = _run(dev, amd, sc)
            record.append("%s %s %s\n" % (sc["name"], row, " ".join(sorted(census))))
        except (AssertionError, amd.api.LC3Error) as e:
            failed.append((sc["name"], row, str(e)[:600]))
            dev.sync()                                                       # a device that no longer answers ends the case here
        dev.free()
    if os.environ.get("LC3PLUS_OPTION_PAIRS_RECORD"):
        with open(os.environ["LC3PLUS_OPTION_PAIRS_RECORD"], "a") as f:
            f.writelines(record)
    for f in failed:
        print("FAILED ROW", f)
    assert not failed, ("rows that differ from the oracle", [f[0] for f in failed], failed[0])


RS_GROUPS = [(g, l) for g in op.RESAMPLE_GEOMS for l in op.LAYOUTS]
RS_TYPED = {"G48S": {"lc3_enc_resample48_kernel", "lc3_enc_resample48f_kernel", "lc3_enc_resample48w_kernel"}, "G96_25S": {"lc3_enc_resample96_kernel_n240"}}


@pytest.mark.parametrize("geom,layout", RS_GROUPS, ids=["%s-%s" % g for g in RS_GROUPS])
def test_resample_rows_equal_the_oracle(dev, geom, layout):
    """option_pairs.RESAMPLE_ROWS: every sample type at every alignment in one layout of a geometry with resamplers of its own.  In the default layout the
    aligned rows must have reached every typed resampler of the geometry and the others the three for every shape: the table keeps reaching the twins it is there for."""
    amd = _amd()
    rows = [(n, row) for n, row in enumerate(op.RESAMPLE_ROWS) if (row[0], row[5]) == (geom, layout)]
    failed, record, seen = [], [], set()
    for n, row in rows:
        sc = op.scenario("enc", n, row, prefix="rs")
        try:
            census = _run(dev, amd, sc)
            record.append("%s %s %s\n" % (sc["name"], row, " ".join(sorted(census))))
            seen |= set(census)
        except (AssertionError, amd.api.LC3Error) as e:
            failed.append((sc["name"], row, str(e)[:600]))
            dev.sync()
        dev.free()
    if os.environ.get("LC3PLUS_OPTION_PAIRS_RECORD"):
        with open(os.environ["LC3PLUS_OPTION_PAIRS_RECORD"], "a") as f:
            f.writelines(record)
    for f in failed:
        print("FAILED ROW", f)
    assert not failed, ("rows that differ from the oracle", [f[0] for f in failed], failed[0])
    if layout == "default":
        want = RS_TYPED[geom] | {"lc3_enc_resample_kernel", "lc3_enc_resample_fmt_kernel", "lc3_enc_resample_wire_kernel"}
        assert want <= seen, sorted(want - seen)


# ---- the refusals ----
def _fmt(api, form, layout):
    return api.pcm_format(api.PCM_FLOAT32 if form == "f32" else form, layout)


def _refused_call(dev, api, side, r, b):
    """the first call of row r (which breaks one clause) on batch b with real buffers: raises LC3Error, writes nothing"""
    fs, ms, hr, ch, rates = op.GEOMS[r["geom"]]
    S, T, N = len(rates), r["calls"][0], b.N
    fmt = _fmt(api, r["form" if side == "enc" else "out"], r["layout"])
    n_pcm = S * T * ch * N * op.ELEM_BYTES[r["form" if side == "enc" else "out"]]
    sizes = [lc.nbytes_of(fs, ch, ms, hr, x) for x in rates]
    stride = max(sizes)
    outs = []

    def sent(shape, dtype, val):
        outs.append((dev.put(np.full(shape, val, dtype)), shape, dtype, val))
        return outs[-1][0]
    if r["placed"]:
        getattr(b, "set_pcm_placement")(dev.put(np.zeros((S, T), np.int64)), S * T * ch * N)
    if r["ragged"]:
        b.set_frame_counts(dev.put(np.full(S, T, np.int32)))
    try:
        with pytest.raises(api.LC3Error):
            if side == "enc":
                br, bw = lc._words(dict(words=r["words"]), fs, rates, S, T, 0, False)
                d_pcm = dev.put(np.zeros(n_pcm, np.uint8))
                if r["how"] == "host":
                    b.encode(np.zeros(api.pcm_shape(fmt, S, T, ch, N), api.pcm_dtype(fmt)), bitdepth=fmt, bitrates=br, bandwidths=bw)
                elif r["how"] in ("device", "hostwords"):
                    b.encode_device(d_pcm, fmt, T, sent((S, T, stride), np.uint8, lc.SENT), stride, sync=True, bitrates=br, bandwidths=bw)
                else:
                    d_br, d_bw = (dev.put(br) if br is not None else None), (dev.put(bw) if bw is not None else None)
                    if r["how"] == "rates":
                        b.encode_device_rates(d_pcm, fmt, T, sent((S, T, stride), np.uint8, lc.SENT), stride, d_br, d_bw, sent((S, T), np.int32, lc.NB_SENT),
                                              sent((S, T), np.uint8, lc.FL_SENT), sync=True)
                    else:
                        b.encode_device_packed(d_pcm, fmt, T, sent((S * T * stride,), np.uint8, lc.SENT), S * T * stride, r["order"], d_br, d_bw,
                                               sent((S, T), np.int64, -99), sent((1,), np.int64, -99), sent((S, T), np.int32, lc.NB_SENT),
                                               sent((S, T), np.uint8, lc.FL_SENT), sync=True)
            else:
                var = r["how"] in ("hostsizes", "devhostsizes", "sizes", "packed")
                nb = np.array(sizes, np.int32)[:, None].repeat(T, axis=1)
                fr = np.zeros((S, T, stride), np.uint8)
                if r["how"] in ("host", "hostsizes"):
                    b.decode(fr, np.zeros((S, T), np.uint8), bps=fmt, num_bytes=nb if var else None)
                elif r["how"] in ("device", "devhostsizes"):
                    b.decode_device(dev.put(fr), stride, T, sent((n_pcm,), np.uint8, 0x5A), bps=fmt, sync=True, num_bytes=nb if var else None)
                elif r["how"] == "sizes":
                    b.decode_device_sizes(dev.put(fr), stride, T, sent((n_pcm,), np.uint8, 0x5A), dev.put(nb), dev.put(np.zeros((S, T), np.uint8)),
                                          sent((S, T), np.uint8, lc.ST_SENT), bps=fmt, sync=True)
                else:
                    po = (np.arange(S * T, dtype=np.int64) * stride).reshape(S, T)
                    b.decode_device_packed(dev.put(np.zeros(S * T * stride, np.uint8)), S * T * stride, dev.put(po), T, sent((n_pcm,), np.uint8, 0x5A), dev.put(nb),
                                           stride, dev.put(np.zeros((S, T), np.uint8)), sent((S, T), np.uint8, lc.ST_SENT), bps=fmt, sync=True)
    finally:
        if r["ragged"]:
            b.set_frame_counts(None)
        if r["placed"]:
            b.set_pcm_placement(None)
    dev.sync()
    for ptr, shape, dtype, val in outs:
        assert (dev.get(ptr, shape, dtype) == val).all(), "a refused call wrote to an output buffer"


def _refusals():
    """(side, clause, the row that breaks it alone, the same row mended at a factor other than the geometry) for the first excluded pair of every refusal clause"""
    out = []
    for side in ("enc", "dec"):
        ex = op.excluded_by_clause(side)
        for c in op.SIDES[side][1]:
            if c.kind != "refusal":
                continue
            r = op.only_breaks(side, ex[c.name][0], c.name)
            mended = [dict(r, **{f: v}) for f in (c.fb, c.fa) if f != "geom" for v in dict(op.SIDES[side][0])[f] if op.valid(side, dict(r, **{f: v}))]
            out.append((side, c.name, r, mended[0]))
    return out


@pytest.mark.parametrize("side,clause,r,mended", _refusals(), ids=["%s-%s" % x[:2] for x in _refusals()])
def test_an_excluded_pair_is_refused_and_leaves_the_batch_as_it_was(dev, side, clause, r, mended):
    amd = _amd()
    assert op.violations(side, r) == [clause] and op.valid(side, mended)
    sc = op.scenario(side, 900, mended)
    sc["before"] = lambda b: _refused_call(dev, amd.api, side, r, b)
    _run(dev, amd, sc)
