"""Poisoned workspaces (test helper beside launch_census.py, TEST INFRASTRUCTURE ONLY): the class of every pointer member of the host runtime's two context structs.

audio_codec_amd/csrc/lc3_runtime.hip keeps a batch's device buffers in struct lc3hip_ctx (encoder) and struct lc3hip_dctx (decoder) and the structs they embed
(lc3hip_stage, lc3hip_ss, work_set).  LC3PLUS_POISON_WORK fills the buffers of class `work`; every other member needs the reason it is left alone:

  work    a call fills it and reads it itself; no later call may rely on it.  Poisoned.  Equal to the runtime's tables enc_work / dec_work.
  state   a later call reads, by design, what an earlier call wrote: the reader is named.
  const   written once (plan, tables, template).
  alias   points into a buffer of another member; owns nothing.
  caller  the caller's device memory, kept for the call being queued or until the caller takes it back.
  host    host memory (pinned staging, malloc, the runtime's own tables).

tests/test_poison_work_cpu.py parses the structs and the two tables from the source text: a buffer added later without a class fails there.
tests/test_gpu_poisoned_work.py runs the library under the switches."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNTIME = os.path.join(ROOT, "audio_codec_amd", "csrc", "lc3_runtime.hip")
EMBEDDED = {"lc3hip_stage", "lc3hip_ss", "work_set"}                # struct types whose members count as the context's own

ENC = {
    # ---- work ----
    "d_pcm": ("work", "lc3hip_encode: staging of a host PCM array, copied in whole before the call's kernels"),
    "d_out": ("work", "lc3hip_encode / encode_host: staging of the frames for a host array, cleared on the call's stream, copied out behind the writer"),
    "d_trace": ("work", "lc3hip_encode: the traces of a traced call, cleared on the call's stream, copied out behind it"),
    "hp_dpcm": ("work", "encode_host: the two chunk slots of a host-pointer call's PCM, each copied in before the piece that reads it"),
    "d_dumpv": ("work", "enc_size_set: the writer's scratch rows (isc scalars, residual bits, quantised spectrum) of the call's set"),
    "d_y12": ("work", "enc_size_set: the 12.8 kHz rows the resampler writes and the HP50, pitch and one-wave kernels of the same call read"),
    "d_statusv": ("work", "enc_size_set: the status bytes of the call's set, cleared per call (hipMemsetAsync: enc_size_set, enc_writer)"),
    "d_spec": ("work", "enc_size_set: the spectrum rows the front writes and the lane, rate and writer kernels of the same call read"),
    "d_frec": ("work", "enc_size_set: the per-frame records of the pipelined path; the padding words are written by no kernel"),
    "d_cnt": ("work", "lc3hip_encode_rates_device: the clamped counts the ragged plan kernel writes, read by the other kernels of that call"),
    "fsz.d": ("work", "upload_fsz: the call's frame sizes, copied from the pinned twin on the call's stream"),
    "bw.d": ("work", "stage_bw / bw_to: the call's bandwidths, copied from the pinned twin or written by the plan kernel's twin buffers"),
    "d_pfsz": ("work", "plan_launch: the sizes the plan kernel of a call writes for that call's kernels"),
    "d_pbw": ("work", "plan_launch: the bandwidths the plan kernel of a call writes for that call's kernels"),
    "d_pend": ("work", "plan_launch: the carry after the call, written by its plan kernel, read by its tail kernel and its scan"),
    "d_poff": ("work", "pack_scan / plan_launch: the table of offsets (or slots) the call's writers read"),
    "d_pbsum": ("work", "pack_scan: the tile sums of the call's scan, written by lc3_pack_sums_kernel, read by the two kernels behind it"),
    # ---- state ----
    "d_state": ("state", "every kernel that carries a stream across frames reads the rows the previous call left (enc_run: c->d_state + LC3D_ST_XPREV; lc3hip_get_state)"),
    "d_chans": ("state", "the configuration: every call's kernels read what lc3hip_upload_chans or an earlier call's tail kernel wrote"),
    "d_carry": ("state", "lc3_enc_plan_rates_kernel of a call reads carry[s], written by the plan kernel of the call before (plan_launch: c->carry_seed ? d_chans : carry)"),
    "d_xnext": ("state", "enc_pipelined: r.xprev = ahead ? c->d_xnext[(xn_par + LC3D_SETS) % (LC3D_SETS + 1)] - the front of the call before wrote it as xn_w"),
    "ss.d": ("state", "ss_run: lc3_stream_state_kernel and an export's copy read the slot after the lifecycle call has returned; encode and decode calls never touch it"),
    # ---- const ----
    "d_plan": ("const", "lc3hip_create: the plan, copied once"),
    "d_etab": ("const", "lc3hip_upload_enc_table: the configuration per byte count, uploaded once before the first call that reads it"),
    "ss.d_tmpl": ("const", "ss_init: the fresh-row template, copied once per lc3hip_set_template"),
    # ---- alias ----
    "d_status": ("alias", "enc_size_set: c->d_status = c->d_statusv[set]"),
    "last_frec": ("alias", "enc_pipelined: c->last_frec = c->d_frec[set], for lc3hip_last_records"),
    "pk.tab": ("alias", "pack_scan / plan_launch: c->pk.tab = c->d_poff[slot]"),
    "bw_src": ("alias", "stage_bw: c->bw_src = c->bw.h[k], pinned host memory"),
    # ---- caller ----
    "plo": ("caller", "lc3hip_set_pcm_placement"),
    "counts": ("caller", "lc3hip_set_frame_counts"),
    "pl.rates": ("caller", "lc3hip_encode_rates_device: rates_dev of the call being queued"),
    "pl.bws": ("caller", "lc3hip_encode_rates_device: bws_dev"),
    "pl.nb": ("caller", "lc3hip_encode_rates_device: num_bytes_dev"),
    "pl.fl": ("caller", "lc3hip_encode_rates_device: flags_dev"),
    "pk.offs": ("caller", "lc3hip_encode_packed: offsets_dev"),
    "pk.total": ("caller", "lc3hip_encode_packed: total_dev"),
    "pk.nb": ("caller", "lc3hip_encode_packed: num_bytes_dev"),
    "pk.fl": ("caller", "lc3hip_encode_packed: flags_dev"),
    # ---- host ----
    "h_attack": ("host", "calloc: chans_host_side_list"),
    "h_nb": ("host", "calloc: chans_host_side_list"),
    "h_chans": ("host", "pinned: lc3hip_upload_chans_async"),
    "hp_pin_in": ("host", "pinned: encode_host"),
    "fsz.h": ("host", "pinned: stage_words"),
    "bw.h": ("host", "pinned: stage_words"),
    "ss.h": ("host", "pinned: ss_run"),
    "wk.ctx": ("host", "the context itself"),
    "wk.tab": ("host", "the table enc_work, in the library's data"),
}

DEC = {
    "d_in": ("work", "dec_stage: staging of a host array of frames, copied in whole before the parser"),
    "d_pcm": ("work", "dec_stage: staging of the samples for a host array, written by the synthesis, copied out behind it"),
    "d_bfi": ("work", "dec_stage / dec_plan: the call's loss flags, copied from the host or written by the plan kernel"),
    "d_sizes": ("work", "dec_stage / dec_plan: the call's frame sizes, copied from the host or written by the plan kernel"),
    "d_inval": ("work", "dec_plan: the call's invalid flags, written by the plan kernel, read by the tail kernel"),
    "d_trace": ("work", "dec_stage: the traces of a traced call, cleared on the call's stream"),
    "d_status": ("work", "dec_stage: the status bytes of a call that returns them to the host, written by the synthesis"),
    "d_rec": ("work", "dec_stage: the records the parser and the concealment kernel write, the transform and the synthesis of the same call read"),
    "d_ws": ("work", "dec_stage: the spectrum rows the parser writes up to the last tuple's group, the transform of the same call reads"),
    "d_ov": ("work", "dec_stage: the transformed frames the IMDCT writes and the synthesis of the same call reads"),
    "d_recx": ("work", "dec_stage: d_rec of the other sets under the input-ready promise"),
    "d_wsx": ("work", "dec_stage: d_ws of the other sets under the input-ready promise"),
    "d_cnt": ("work", "dec_plan: the clamped counts the ragged plan kernel writes, read by the other kernels of that call"),
    "d_state": ("state", "lc3_dec_plc_kernel, the IMDCT and the synthesis read the rows the previous call left (dec_chain; lc3hip_dec_get_state)"),
    "d_chans": ("state", "the configuration: dec_parse reads what lc3hip_dec_upload_chans or an earlier call's lc3_dec_sizes_tail_kernel wrote"),
    "ss.d": ("state", "ss_run: as the encoder's"),
    "d_plan": ("const", "lc3hip_dec_create: the plan, copied once"),
    "d_tab": ("const", "lc3hip_dec_upload_table: the configuration per byte count, uploaded once"),
    "ss.d_tmpl": ("const", "ss_init: the fresh-row template, copied once"),
    "plo": ("caller", "lc3hip_dec_set_pcm_placement"),
    "counts": ("caller", "lc3hip_dec_set_frame_counts"),
    "h_nbytes": ("host", "calloc: dec_note_nbytes"),
    "ss.h": ("host", "pinned: ss_run"),
    "wk.ctx": ("host", "the context itself"),
    "wk.tab": ("host", "the table dec_work, in the library's data"),
}

CLASSES = {"lc3hip_ctx": ENC, "lc3hip_dctx": DEC}
TABLES = {"lc3hip_ctx": "enc_work", "lc3hip_dctx": "dec_work"}


def source():
    with open(RUNTIME) as f:
        return f.read()


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _body(text, head):
    """the text between the braces that follow `head`"""
    at = text.index(head)
    a = text.index("{", at)
    depth, i = 0, a
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[a + 1:i], i + 1
        i += 1


def _members(text, name, prefix=""):
    """every pointer member of struct `name`, members of embedded and anonymous structs with their path: ["d_plan", "fsz.d", "pl.rates", ...]"""
    body, _ = _body(text, "struct %s {" % name)
    return _members_of(text, body, prefix)


def _members_of(text, body, prefix):
    out = []
    while "struct {" in body:                                        # anonymous structs: `struct { ... } pl;`
        inner, end = _body(body, "struct {")
        var = re.match(r"\s*(\w+)\s*;", body[end:])
        out += _members_of(text, inner, prefix + var.group(1) + ".")
        body = body[:body.index("struct {")] + body[end + var.end():]
    for decl in body.split(";"):
        decl = decl.strip()
        m = re.match(r"(?:const\s+)?(\w+)\s+(\w+)(\s*\[[^\]]*\])?$", decl)
        if m and m.group(1) in EMBEDDED:                             # `lc3hip_stage fsz`, `lc3hip_ss ss`, `work_set wk`
            out += _members(text, m.group(1), prefix + m.group(2) + ".")
            continue
        if "*" not in decl or "(" in decl:
            continue
        first, _, rest = decl.partition("*")                        # `const long long` * `plo`  |  `float` * `d_spec[LC3D_SETS]`
        names = [rest] + [d[1:] for d in (x.strip() for x in rest.split(",")[1:]) if d.startswith("*")]
        names[0] = names[0].split(",")[0]
        for n in names:
            out.append(prefix + re.match(r"\s*\**\s*(\w+)", n).group(1))
    return out


def pointer_members(ctx):
    return _members(_strip_comments(source()), ctx)


def table(ctx):
    """the runtime's enumerator table of a context struct from the source text: [(member, count expression, element type)]"""
    body, _ = _body(_strip_comments(source()), "static const work_buf %s[] =" % TABLES[ctx])
    rows = re.findall(r"WORK\(\s*(\w+)\s*,\s*([\w.]+)\s*,\s*([^,]+?)\s*,\s*LC3HIP_ELEM_(\w+)\s*,", body)
    assert all(r[0] == ctx for r in rows), rows
    return [(r[1], r[2], r[3]) for r in rows]


def work_members(ctx):
    return sorted(k for k, (cls, _) in CLASSES[ctx].items() if cls == "work")
