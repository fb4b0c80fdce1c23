"""Which frames of tests/hostile_frames.py test which "conceal this frame" decision: builds eleven copies of the CPU oracle decoder in a temporary directory, each
with ONE of the decisions of dec_side / dec_spectrum taken out (oracle/lc3_oracle_dec.inc, by text substitution: the script stops if a line it replaces is no
longer there), and counts per geometry the frames refused for that reason that the copy accepts.  A parser that loses the same decision decodes exactly those
frames, so every test of tests/test_gpu_hostile_frames.py on their geometry fails on status and PCM.  CPU only; DESIGN.md section 8 quotes the output.
Usage: python tools/oracle_mutants.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostile_frames as hf                                      # noqa: E402
import lc3_harness as lh                                         # noqa: E402

SRC = os.path.join(ROOT, "oracle")
NOBER = ("if (st->low >= (uint32_t)(tmp << 10)) st->ber = 1;", "")          # in a second copy of ad_decode: the state check of the range decoder left out
# reason -> substitutions.  lastnz and nres are clamped instead of dropped, so that the copy stays inside its arrays.
MUTANTS = {
    hf.REJ_BANDWIDTH: [("if (d->fs_idx < *bw) { LC3O_REJECT(LC3O_REJ_BANDWIDTH); return 1; }", "")],
    hf.REJ_LASTNZ: [("    if (*lastnz > d->ylen) { LC3O_REJECT(LC3O_REJ_LASTNZ); return 1; }", "    if (*lastnz > d->ylen) *lastnz = d->ylen;")],
    hf.REJ_SNS_25: [("        if (t >= 33460056) { LC3O_REJECT(LC3O_REJ_SNS_INDEX_25); return 1; }", "")],
    hf.REJ_SNS_24: [("        if (t >= 16708096) { LC3O_REJECT(LC3O_REJ_SNS_INDEX_24); return 1; }", "")],
    hf.REJ_TNS_ORDER: [("if (tns_order[n] > maxlag) { st.ber = 1; LC3O_BER(LC3O_REJ_TNS_ORDER); }", "")],
    hf.REJ_TNS_READER: [("            if (r->bp < st.bp) { LC3O_REJECT(LC3O_REJ_TNS_READER); return 1; }\n", "")],
    hf.REJ_TNS_SYMBOL: [("ad_decode(&st, &lc3t_tns_order_cum", "ad_decode_nober(&st, &lc3t_tns_order_cum"),
                        ("ad_decode(&st, &lc3t_tns_coef_cum", "ad_decode_nober(&st, &lc3t_tns_coef_cum")],
    hf.REJ_OVERLAP: [("        if (st.bp - r->bp > 3) { LC3O_REJECT(LC3O_REJ_OVERLAP); return 1; }", "")],
    hf.REJ_SPEC_SYMBOL: [("sym = ad_decode(&st, &lc3t_ac_cum", "sym = ad_decode_nober(&st, &lc3t_ac_cum")],
    hf.REJ_ESCAPE_14: [("if ((lev - 1) == 13 && sym == 16) { st.ber = 1; LC3O_BER(LC3O_REJ_ESCAPE_14); }", "")],
    hf.REJ_NRES: [("    if (*nres < 0) { LC3O_REJECT(LC3O_REJ_NRES); return 1; }", "    if (*nres < 0) *nres = 0;")],
}


def build(reason, where):
    base = open(os.path.join(SRC, "lc3_oracle_dec.inc")).read()
    ad = base[base.index("static int ad_decode("):base.index("/* R/ari_codec.c:204-509.")]
    assert ad.count(NOBER[0]) == 1
    s = base.replace(ad, ad + ad.replace("static int ad_decode(", "static int ad_decode_nober(").replace(*NOBER))
    for a, b in MUTANTS[reason]:
        assert s.count(a) == 1, (reason, a)
        s = s.replace(a, b)
    os.makedirs(where)
    for f in os.listdir(SRC):
        if f.endswith((".c", ".h", ".inc")):
            open(os.path.join(where, f), "w").write(s if f == "lc3_oracle_dec.inc" else open(os.path.join(SRC, f)).read())
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fPIC", "-w", "-I" + os.path.join(ROOT, "audio_codec_amd", "csrc"),
                           "-DLC3O_PORTABLE_MATH=1", "-shared", "-o", os.path.join(where, "liblc3_oracle_pm.so"), os.path.join(where, "lc3_oracle.c"), "-lm"])


def run():
    """-> {reason: {geometry: (frames the copy accepts, frames refused for the reason)}}"""
    streams = {g: hf.streams(g) for g in hf.GEOMS}                # with the real oracle, before ORACLE_DIR moves
    out, real = {}, lh.ORACLE_DIR
    with tempfile.TemporaryDirectory() as td:
        for r in hf.REASONS:
            build(r, os.path.join(td, "m%d" % r))
            lh.ORACLE_DIR = os.path.join(td, "m%d" % r)
            try:
                out[r] = {}
                for g, (frames, sizes, bfi, kind, reason) in streams.items():
                    fs, ms, hr, ch, _ = hf.GEOMS[g]
                    full = hf.stream_sizes(g)
                    d = lh.OracleDecoder(fs, 1, ms, hr, portable_math=True)
                    n = tot = 0
                    for i, t in np.argwhere(reason == r):
                        b, c = divmod(int(i), ch)
                        z = hf.channel_sizes(int(full[b, t]), ch)
                        rc, _ = d.decode(frames[b, t, sum(z[:c]):sum(z[:c + 1])])
                        tot += 1; n += rc == 0
                    if tot:
                        out[r][g] = (n, tot)
            finally:
                lh.ORACLE_DIR = real
    return out


if __name__ == "__main__":
    names = lh.reject_names()
    for r, per in run().items():
        print("%-13s accepted without the check: %3d of %3d   " % (names[r], sum(a for a, _ in per.values()), sum(b for _, b in per.values()))
              + "; ".join("%s %d/%d" % (g, a, b) for g, (a, b) in per.items()))
